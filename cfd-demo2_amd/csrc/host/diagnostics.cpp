// Flow diagnostics of the current state (kernels.hpp FlowDiagArgs): scalars,
// derived cell fields, the wall-force region and the reference's adaptive
// time-step rule (src/ui/app.rs:871-910) without a velocity read-back.
#include <cmath>
#include <cstring>
#include <limits>

#include "solver_impl.hpp"

namespace cfd2 {

// The reference's driver loop (app.rs:897-909) in f64: nothing happens unless
// max_vel > 1e-6; target_cfl * min_cell_size / max_vel, at most 1.2 x the
// current dt, clamped to [1e-9, 100].
bool adaptive_dt_rule(double current_dt, double target_cfl, double min_cell_size, double max_vel, double* next_dt) {
  if (!(max_vel > 1e-6)) {
    *next_dt = current_dt;
    return false;
  }
  double next = target_cfl * min_cell_size / max_vel;
  if (next > current_dt * 1.2) next = current_dt * 1.2;
  if (next < 1e-9) next = 1e-9;  // f64::clamp: a NaN stays a NaN
  if (next > 100.0) next = 100.0;
  *next_dt = next;
  return true;
}

void Solver::flow_diag_alloc(bool fields) {
  const uint32_t nb = red_blocks(N);
  if (!diag_partial) {
    diag_partial = arena.alloc<double>((size_t)kFlowDiagSums * pstride);
    diag_blockmax = arena.alloc<unsigned long long>(3 * (size_t)nb);
    diag_res = arena.alloc<uint64_t>(9 + 3 * (size_t)R);
    if (dist()) {
      diag_red_local = arena.alloc<double>((size_t)kFlowDiagSums * maxseg);
      diag_red_gather = arena.alloc<double>((size_t)R * kFlowDiagSums * maxseg);
    }
  }
  if (fields && !diag_omega) {
    diag_omega = arena.alloc<float>(N);
    diag_div = arena.alloc<float>(N);
  }
}

void Solver::flow_diag_device(bool fields, bool reduce) {
  flow_diag_alloc(fields);
  FlowDiagArgs a{};
  a.N = N;
  a.c = constants;
  a.fs = fs;
  a.vol = d_vol;
  a.u = S().u;
  a.p = S().p;
  a.wall_mask = region.on ? region.mask : nullptr;
  a.omega_out = fields ? diag_omega : nullptr;
  a.div_out = fields ? diag_div : nullptr;
  a.out = sums().out(diag_partial);
  a.blockmax = diag_blockmax;
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(diag_res + 6);
  // prescribed boundary velocities: the moving walls' face values and relative velocity
  const BcvArgs v = bcv.args();
  launch_flow_diag(a, bcv.on() ? &v : nullptr, visc.mu, mx, stream);
  if (!reduce) {  // derived fields only: nothing to reduce across ranks, not collective
    check_launch("flow diagnostics (fields)");
    return;
  }
  launch_evolution_final(combine(diag_partial, kFlowDiagSums, diag_red_local, diag_red_gather),
                         reinterpret_cast<double*>(diag_res), stream);
  if (dist()) {
    const CommScope scope(this, kCommReduceGather);
    timed_gather(kCommReduceGather, 3 * sizeof(uint64_t),
                 [&] { comm->allgather(diag_res + 6, diag_res + 9, 3 * sizeof(uint64_t), stream); });
  }
  check_launch("flow diagnostics");
}

void flow_diag_decode(const uint64_t* sumbits, const uint64_t* m, uint32_t faces, cfd_flow_diag* out) {
  double sums[kFlowDiagSums], smax;
  std::memcpy(sums, sumbits, sizeof(sums));
  std::memcpy(&smax, &m[0], sizeof(double));
  const uint32_t ob = (uint32_t)m[1], db = (uint32_t)m[2];
  float omax, dmax;
  std::memcpy(&omax, &ob, 4);
  std::memcpy(&dmax, &db, 4);
  std::memset(out, 0, sizeof(*out));
  out->max_speed = std::sqrt(smax);
  out->max_vorticity = omax;
  out->max_divergence = dmax;
  out->kinetic_energy = sums[0];
  out->enstrophy = sums[1];
  out->force_pressure[0] = sums[2];
  out->force_pressure[1] = sums[3];
  out->force_viscous[0] = sums[4];
  out->force_viscous[1] = sums[5];
  out->region_faces = faces;
}

void Solver::flow_diagnostics(cfd_flow_diag* out, bool fields) {
  const Range range("flow diagnostics");
  CFD_HIP(hipSetDevice(device));
  flow_diag_device(fields, out != nullptr);
  if (!out) return;
  std::vector<uint64_t> h(9 + 3 * (size_t)R);
  CFD_HIP(hipMemcpyAsync(h.data(), diag_res, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  sync();
  uint64_t m[3] = {0, 0, 0};
  const uint64_t* src = dist() ? h.data() + 9 : h.data() + 6;
  for (int q = 0; q < R; ++q)  // rank order (a maximum of bit patterns: any order gives the same)
    for (int j = 0; j < 3; ++j) m[j] = std::max(m[j], src[3 * q + j]);
  flow_diag_decode(h.data(), m, region.faces, out);
}

void Solver::get_derived(int kind, double* out) {
  if (kind < 0 || kind > 2) throw std::invalid_argument("derived field kind must be 0 (speed), 1 (vorticity) or 2 (divergence)");
  CFD_HIP(hipSetDevice(device));
  if (kind == 0) {  // |u| in f64 from the f32 state: the reference's per-cell v (app.rs:891)
    std::vector<float2> u(N);
    CFD_HIP(hipMemcpyAsync(u.data(), S().u, N * sizeof(float2), hipMemcpyDeviceToHost, stream));
    sync();
    for (uint32_t i = 0; i < N; ++i)
      out[i] = std::sqrt((double)u[i].x * (double)u[i].x + (double)u[i].y * (double)u[i].y);
    return;
  }
  flow_diagnostics(nullptr, true);
  std::vector<float> f(N);
  CFD_HIP(hipMemcpyAsync(f.data(), kind == 1 ? diag_omega : diag_div, N * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) out[i] = f[i];
}

uint32_t Solver::set_force_region(double x0, double y0, double x1, double y1) {
  CFD_HIP(hipSetDevice(device));
  std::vector<uint16_t> mask;
  uint32_t count = 0;
  for (const uint32_t j : wall_faces_in_box(wall_faces, x0, y0, x1, y1)) {
    const WallFace& wfc = wall_faces[j];
    ++count;
    if (wfc.cell < topo.c0 || wfc.cell >= topo.c1) continue;
    if (wfc.slot >= 16) throw std::invalid_argument("force region: wall face beyond slot 15 of its cell");
    if (mask.empty()) mask.assign(N, 0);
    mask[wfc.cell - topo.c0] |= (uint16_t)(1u << wfc.slot);
  }
  region.faces = count;
  ++region.gen;  // wall_motion rebuilds its table of face centres
  region.box[0] = x0, region.box[1] = y0, region.box[2] = x1, region.box[3] = y1;
  region.on = count != 0;  // every rank runs the same kernel form (the force sums of a rank without faces are +0)
  if (!region.on) return 0;
  if (mask.empty()) mask.assign(N, 0);
  if (!region.mask) region.mask = arena.alloc<uint16_t>(N);
  CFD_HIP(hipMemcpyAsync(region.mask, mask.data(), (size_t)N * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
  sync();
  return count;
}

// ---- the module calls that run the diagnostics first ----
void Solver::render(int32_t field, int32_t scalar_index, const float* range, uint8_t* rgba, float* used) {
  const FlowView flow = view(Renderer::kOneGpu);
  renderer.frame_check(flow, field, scalar_index);
  const Range rr("render");
  const float* derived = nullptr;
  if (field == 4 || field == 5) {
    flow_diagnostics(nullptr, true);  // the derived pass, its field outputs on
    derived = field == 4 ? diag_omega : diag_div;
  }
  renderer.frame(flow, field, scalar_index, derived, range, rgba, used);
}

void Solver::monitor_enable(uint32_t capacity, uint32_t num_probes, const uint32_t* cells, bool with_diag) {
  monitor.enable(view(Monitor::kOneGpu), capacity, num_probes, cells, with_diag);
  if (with_diag) flow_diag_alloc(false);  // the record itself allocates nothing
}

void Solver::monitor_record() {
  const FlowView flow = view(Monitor::kOneGpu);
  monitor.record_check(flow);
  const Range range("monitor record");
  CFD_HIP(hipSetDevice(device));
  if (monitor.diag) flow_diag_device(false, true);
  monitor.record(flow, diag_res, region);
}

float Solver::adapt_dt(double target_cfl) {
  cfd_flow_diag d;
  flow_diagnostics(&d);
  double next = 0.0;
  if (adaptive_dt_rule((double)constants.dt, target_cfl, min_cell, d.max_speed, &next)) {
    const float dt = (float)next;
    constants.dt_old = (constants.dt > 0.0f) ? constants.dt : dt;  // cfd_set_dt (solver.rs:36-44)
    constants.dt = dt;
  }
  return constants.dt;
}

}  // namespace cfd2
