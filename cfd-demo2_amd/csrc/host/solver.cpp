// Host driver of the HIP coupled step: restates the control flow of
//   coupled_solver.rs:33-580            step_coupled / check_evolution (here)
//   solver.rs:9-44, 97-128, 276-294     set_u / set_p / set_dt / getters / history (here)
//   init/fields.rs:62-139               fields and constants (the constructor)
//   coupled_solver_fgmres.rs:1728-2448  solve_coupled_fgmres (fgmres.cpp)
//   async_buffer.rs                     the lagged reads (LagReader, solver_impl.hpp)
//   coupled_solver_fgmres.rs:174-209    ensure_amg_resources (amg_levels.cpp)
//   linear_solver/amg.rs:84-235, 374-595  the hierarchy (amg_setup.cpp, amg_device.cpp)
//   linear_solver/amg.rs:666-770        v_cycle (amg_cycle.cpp)
// over the kernels of ../hip/*.hip, on one HIP stream.  All vectors stay
// in HBM; the step's own host round trips are the lagged max-diff reads and
// check_evolution's five sums.  Also: halo.cpp, debug.cpp, accounting.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <cstring>
#include <limits>

#include "solver_impl.hpp"

namespace cfd2 {

// Rust's `{:.2e}` (the reference's log format): 1.23e-5, 3.40e38, NaN, inf
std::string e2(double v) {
  if (std::isnan(v)) return "NaN";
  if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[48];
  std::snprintf(buf, sizeof(buf), "%.2e", v);
  const std::string s(buf);
  const size_t e = s.find('e');
  size_t i = e + 1;
  const bool neg = s[i] == '-';
  if (s[i] == '-' || s[i] == '+') ++i;
  while (i + 1 < s.size() && s[i] == '0') ++i;
  return s.substr(0, e) + "e" + (neg ? "-" : "") + s.substr(i);
}

Solver::Solver(const cfd_mesh_view& mesh, const cfd_config& c, int dev, std::unique_ptr<Comm> cm)
    : cfg(c), device(dev) {
  if (cfg.max_restart < 1 || cfg.max_restart > 63) throw std::invalid_argument("max_restart must be 1..63");
  m = cfg.max_restart;
  m1 = m + 1;
  NG = mesh.num_cells;
  if (cm && cm->size > 1) {
    comm = std::move(cm);
    R = comm->size;
    rk = comm->rank;
  }
  starts = partition_starts(NG, R);
  build_topology(mesh, topo, (uint32_t)starts[rk], (uint32_t)starts[rk + 1]);
  N = topo.N;
  F = topo.F;
  // flow diagnostics (diagnostics.cpp): the host data the mesh view is needed for
  min_cell = std::numeric_limits<double>::infinity();
  for (uint32_t i = 0; i < NG; ++i) min_cell = std::fmin(min_cell, std::sqrt(mesh.cell_vol[i]));
  for (uint32_t i = 0; i < NG; ++i)
    for (uint32_t k = mesh.cell_face_offsets[i]; k < mesh.cell_face_offsets[i + 1]; ++k) {
      const uint32_t f = mesh.cell_faces[k];
      if (f >= mesh.num_faces) throw std::invalid_argument("cell_faces out of range");
      if (mesh.face_neighbor[f] == UINT32_MAX && (mesh.face_boundary[f] & 3u) == 3u)
        wall_faces.push_back({mesh.face_cx[f], mesh.face_cy[f], i, k - mesh.cell_face_offsets[i]});
    }
  if (R == 1) {  // the opt-in physics (one GPU only): boundary faces; the source box tests the f64 centres
    bcv.faces = boundary_faces(mesh);
    cell_cx.assign(mesh.cell_cx, mesh.cell_cx + NG);
    cell_cy.assign(mesh.cell_cy, mesh.cell_cy + NG);
  }
  red = red_geom(NG);
  if (red.nseg > kRedMaxSegments)
    throw std::invalid_argument("mesh too large for the reduction tree (at most 268 M cells)");
  nchunks = (N + kRedChunkCells - 1) / kRedChunkCells;
  nunits = (nchunks + red.U - 1) / red.U;
  pstride = (nunits + 3) & ~3u;
  shift = (topo.glo + 63) & ~63u;
  vlen = (size_t)shift + topo.npad + topo.ghi;
  CFD_HIP(hipSetDevice(device));
  lds_budget = init_kernel_attributes(device);
  amg_wide_limit = (int)std::max<uint64_t>(1, std::min<uint64_t>(255, knob_u64(Knob::AmgWideLimit, 255)));
  check_sync = cfg.log_level >= 3;  // debug: synchronise and check after every launch
  small_forms = knob_on(Knob::SmallMeshForms);
  nt_mask = (unsigned)knob_u64(Knob::Nt, nt_mask);
  // C1-size meshes: 64 MB of the dots pass kept in the Infinity Cache for a
  // top-down update (profiles/r04/ab_cgskeep2_c1.txt: update 36.5-36.9 ->
  // 32.3 us, dots +0.3 us per iteration); from 2^22 cells on the kept lines
  // cost more than they return (ab_cgskeep_c2.txt: dots 284 -> 293 us)
  cgs_keep_bytes = !cgs_serial_form(N) ? (size_t)64 << 20 : 0;
  CFD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  amg_local = dist() && cfg.amg_local_aggregation != 0;
  // hipGraph replay: opt-in through cfd_graph_enable (replay measured no faster
  // than eager launches on this pool, profiles/r05/ab_graph_c0_c1.txt: C0
  // 13.36-13.47 vs 13.30-13.51 ms/step, C1 39.6-39.9 vs 38.8-39.1); halo
  // exchanges and collectives stay eager
  graph_on = false;
  if (dist()) {
    overlap_min_rows = (uint32_t)knob_u64(Knob::OverlapMinRows, overlap_min_rows);
    CFD_HIP(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
    CFD_HIP(hipEventCreateWithFlags(&hev_pack, hipEventDisableTiming));
    CFD_HIP(hipEventCreateWithFlags(&hev_done, hipEventDisableTiming));
    cell_plan = build_halo_plan(starts, rk, topo.srow.data(), N, topo.scol.data(), topo.ghost, topo.glo,
                                topo.npad);
    make_plan_buffers(cell_plan, 8);
    // segments of every rank (ranks own whole segments: partition_starts)
    std::vector<uint32_t> src(red.nseg);
    for (int q = 0; q < R; ++q) {
      const uint64_t s0 = starts[q] / red.seg_cells;
      const uint64_t s1 = (starts[q + 1] + red.seg_cells - 1) / red.seg_cells;
      maxseg = std::max(maxseg, (uint32_t)(s1 - s0));
      for (uint64_t sg = s0; sg < s1; ++sg) src[sg] = ((uint32_t)q << 20) | (uint32_t)(sg - s0);
    }
    if (maxseg >= (1u << 20) || R >= (1 << 12)) throw std::invalid_argument("too many segments / ranks");
    d_seg_src = arena.upload(src, stream);
    red_local = arena.alloc<float>((size_t)m1 * maxseg);
    red_gather = arena.alloc<float>((size_t)R * m1 * maxseg);
    red_local_d = arena.alloc<double>((size_t)5 * maxseg);
    red_gather_d = arena.alloc<double>((size_t)R * 5 * maxseg);
    mx_gather = arena.alloc<uint32_t>(2 * (size_t)R);
    d_u64 = arena.alloc<uint64_t>((size_t)R + 1);  // not lazily: the AMG build runs on amg_arena
    // check_evolution's stride bug reads records (i >> 2) of the global state
    ev_a = (uint64_t)topo.c0 >> 2;
    ev_b = (((uint64_t)topo.c1 - 1) >> 2) + 1;
    const size_t ne = ev_b - ev_a;
    evrec = {arena.alloc<float2>(ne), arena.alloc<float>(ne), arena.alloc<float>(ne), arena.alloc<float2>(ne)};
  }
  // static mesh data
  d_vol = arena.upload(topo.vol, stream);
  fs.other = arena.upload(topo.fs_other, stream);
  fs.meta = arena.upload(topo.fs_meta, stream);
  fs.area = arena.upload(topo.fs_area, stream);
  fs.nx = arena.upload(topo.fs_nx, stream);
  fs.ny = arena.upload(topo.fs_ny, stream);
  fs.lam_s = arena.upload(topo.fs_lam_s, stream);
  fs.lam_f = arena.upload(topo.fs_lam_f, stream);
  fs.dist_a = arena.upload(topo.fs_dist_a, stream);
  fs.dist_e = arena.upload(topo.fs_dist_e, stream);
  fs.dvx = arena.upload(topo.fs_dvx, stream);
  fs.dvy = arena.upload(topo.fs_dvy, stream);
  fs.rx = arena.upload(topo.fs_rx, stream);
  fs.ry = arena.upload(topo.fs_ry, stream);
  fs.rox = arena.upload(topo.fs_rox, stream);
  fs.roy = arena.upload(topo.fs_roy, stream);
  fs.nface = arena.upload(topo.nface, stream);
  fs.wf = topo.wf;
  d_scol = arena.upload(topo.ell_col, stream);
  d_slen = arena.upload(topo.ell_len, stream);
  d_sdrank = arena.upload(topo.ell_drank, stream);
  if (topo.use16) d_scol16 = arena.upload(topo.ell_col16, stream);
  d_slen8 = arena.upload(topo.ell_len8, stream);
  d_sdrank8 = arena.upload(topo.ell_drank8, stream);
  if (topo.use16)
    d_tcol16 = arena.upload(topo.tcol16, stream);
  else
    d_tcol = arena.upload(topo.tcol, stream);
  d_tlg = arena.upload(topo.tlg, stream);
  d_tdrank8 = arena.upload(topo.tdrank8, stream);
  // fields (init/fields.rs:62-139): zero-initialised, with ghost space
  auto zeros_state = [&]() -> StateView {  // u, p, dp, gp: allocated in this order
    return {valloc<float2>(1), valloc<float>(1), valloc<float>(1), valloc<float2>(1)};
  };
  for (auto& r : ring) r = zeros_state();
  prev = zeros_state();
  dp_scratch = valloc<float>(1);
  gp_scratch = valloc<float2>(1);
  const size_t slots_f = (size_t)topo.wf * N, slots_s = (size_t)topo.ws * topo.ld;
  flux_s = arena.alloc<float>(slots_f);
  CFD_HIP(hipMemsetAsync(flux_s, 0, slots_f * sizeof(float), stream));
  grad_u = valloc<float2>(1);
  grad_v = valloc<float2>(1);
  cval_a = arena.alloc<float2>(slots_s);
  cval_g = arena.alloc<float2>(slots_s);
  CFD_HIP(hipMemsetAsync(cval_a, 0, slots_s * sizeof(float2), stream));
  CFD_HIP(hipMemsetAsync(cval_g, 0, slots_s * sizeof(float2), stream));
  cdiag2 = arena.alloc<float2>(topo.ld);
  CFD_HIP(hipMemsetAsync(cdiag2, 0, topo.ld * sizeof(float2), stream));
  sval = arena.alloc<float>(slots_s);
  CFD_HIP(hipMemsetAsync(sval, 0, slots_s * sizeof(float), stream));
  rhs = valloc<float>(3);
  x = valloc<float>(3);
  dinv_uv = valloc<float>(1);
  dinv_p = valloc<float>(1);
  partial_d = arena.alloc<double>(5 * (size_t)pstride + 5);
  maxbits = arena.alloc<uint32_t>(4);
  blockmax = arena.alloc<uint32_t>(2 * (((size_t)N + 255) / 256) + 2);
  // pinned, mapped (for every device: portable) and coherent: kernels may store
  // the per-iteration residual into it directly (d_pin, the device view),
  // visible to the host after the event
  CFD_HIP(hipHostMalloc((void**)&h_pin, 4096 * sizeof(float),
                        hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable));
  CFD_HIP(hipHostGetDevicePointer((void**)&d_pin, h_pin, 0));
  outer.create(2, h_pin + kPinOuter);
  // constants (init/fields.rs:100-115)
  constants.dt = 0.0001f;
  constants.dt_old = 0.0001f;
  constants.time = 0.0f;
  constants.viscosity = 0.01f;
  constants.density = 1.0f;
  constants.component = 0;
  constants.alpha_p = 1.0f;
  constants.scheme = 0;
  constants.alpha_u = 0.7f;
  constants.stride_x = 65535u * 64u;
  constants.time_scheme = 0;
  constants.inlet_velocity = 1.0f;
  constants.ramp_time = 0.1f;
  constants.precond_type = 0;
  std::memset(&info, 0, sizeof(info));
  sync();
}

FlowView Solver::view(const char* one_gpu_message) const {
  if (one_gpu_message && dist()) throw std::invalid_argument(one_gpu_message);
  auto field = [&](int f) { return scalars.surface_field(f, constants.density); };
  return FlowView{device,           stream,           dist(),          N,
                  NG,               topo.ld,          fs,              d_vol,
                  flux_s,           sums(),           constants,       ring[i_state].u,
                  ring[i_state].p,  scalars.s.count,  {field(0), field(1), field(2), field(3)},
                  last_step_dt,     bcv.args(),       bcv.on(),        visc.mu,
                  scalars.gen + bcv.gen,             check_sync};
}

Solver::~Solver() {
  if (stream) (void)hipStreamSynchronize(stream);
  for (IterGraph& G : graphs) {
    if (G.exec) (void)hipGraphExecDestroy(G.exec);
    for (auto e : G.ev) (void)hipEventDestroy(e);
  }
  inner.destroy();
  outer.destroy();
  for (auto e : prof_ev) (void)hipEventDestroy(e);
  if (cstream) (void)hipStreamSynchronize(cstream);
  for (auto e : comm_ev_pool) (void)hipEventDestroy(e);
  if (h_pin) (void)hipHostFree(h_pin);
  if (cstream) (void)hipStreamSynchronize(cstream);
  if (hev_pack) (void)hipEventDestroy(hev_pack);
  if (hev_done) (void)hipEventDestroy(hev_done);
  comm.reset();
  arena.release();
  bcv.arena.release();
  bcv.wm_arena.release();
  visc.arena.release();
  pen.arena.release();
  amg_arena.release();
  scalars.arena.release();
  if (cstream) (void)hipStreamDestroy(cstream);
  if (stream) (void)hipStreamDestroy(stream);
}

CoupledMatrix Solver::cmat() const {
  CoupledMatrix A;
  A.N = N;
  A.r0 = 0;
  A.r1 = N;
  A.r2 = A.r3 = 0;
  A.ld = topo.ld;
  A.ws = topo.ws;
  A.use16 = topo.use16 ? 1 : 0;
  A.col = d_tcol;
  A.col16 = d_tcol16;
  A.lg = d_tlg;
  A.drank = d_tdrank8;
  A.cval_a = cval_a;
  A.cval_g = cval_g;
  A.cdiag2 = cdiag2;
  A.reg = !topo.tmode.empty() && topo.ws <= kCoupledRegMaxWs ? 1 : 0;
  for (int r = 0; r < 8; ++r) A.tmode[r] = r < (int)topo.tmode.size() ? topo.tmode[r] : 0;
  return A;
}

void Solver::log(const char* fmt, ...) const {
  if (cfg.log_level < 1 || rk != 0) return;
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------- state API
// set_u / set_p take the GLOBAL per-cell arrays; a distributed rank keeps its
// owned cells and ghosts.  Getters return the owned cells.
void Solver::set_state(const double* g, int comps_g, const float* field) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float> img;
  local_image(g, comps_g, img);
  for_each_field(S(), [&](float* base, int comps) {
    const size_t bytes = vlen * comps * sizeof(float);
    if (base == field)
      CFD_HIP(hipMemcpyAsync(vbase(base, comps), img.data(), bytes, hipMemcpyHostToDevice, stream));
    else
      CFD_HIP(hipMemsetAsync(vbase(base, comps), 0, bytes, stream));
  });
  sync();
}

// solver.rs:9-21, 23-34: either setter clobbers the whole state
void Solver::set_u(const double* uv) { set_state(uv, 2, reinterpret_cast<float*>(S().u)); }
void Solver::set_p(const double* pv) { set_state(pv, 1, S().p); }

// dst = src over n cells from `off` cells below the owned base
static void copy_state(const StateView& src, StateView& dst, size_t off, size_t n, hipStream_t s) {
  for_each_field(dst, src, [&](float* to, const float* from, int c) {
    CFD_HIP(hipMemcpyAsync(to - off * c, from - off * c, n * c * sizeof(float), hipMemcpyDeviceToDevice, s));
  });
}

void Solver::initialize_history() {  // solver.rs:276-294
  CFD_HIP(hipSetDevice(device));
  copy_state(ring[i_state], ring[i_old], shift, vlen, stream);
  copy_state(ring[i_state], ring[i_old_old], shift, vlen, stream);
  sync();
}

void Solver::get_u(double* uv) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float2> u(N);
  CFD_HIP(hipMemcpyAsync(u.data(), S().u, N * sizeof(float2), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) {
    uv[2 * i] = u[i].x;
    uv[2 * i + 1] = u[i].y;
  }
}

void Solver::get_cells(const float* src, double* out) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float> p(N);
  CFD_HIP(hipMemcpyAsync(p.data(), src, N * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) out[i] = p[i];
}

void Solver::get_p(double* out) { get_cells(S().p, out); }
void Solver::get_d_p(double* out) { get_cells(S().dp, out); }

// ------------------------------------------------------------------ kernels
void Solver::rotate() {  // coupled_solver.rs:43-71
  step_index = (step_index + 1) % 3;
  static const int tab[3][3] = {{0, 1, 2}, {2, 0, 1}, {1, 2, 0}};
  i_state = tab[step_index][0];
  i_old = tab[step_index][1];
  i_old_old = tab[step_index][2];
}

void Solver::prepare() {
  PrepareArgs a;
  a.N = N;
  a.c = constants;
  a.fs = fs;
  a.vol = d_vol;
  a.st = S();
  a.dp_out = dp_scratch;
  a.gp_out = gp_scratch;
  a.flux_s = flux_s;
  a.grad_u = grad_u;
  a.grad_v = grad_v;
  if (ref_racy) {  // test mode: in place, workgroups in order, the owners' fluxes
    a.dp_out = S().dp;
    a.gp_out = S().gp;
    launch_prepare_ordered(a, d_flux_mirror, (uint32_t)((size_t)topo.wf * N), stream);
    check_launch("prepare (reference semantics)");
    return;
  }
  const BcvArgs v = bcv.args();
  if (pen.on())  // volume penalisation (penalty.cpp): the PEN form of whichever of the four is on
    launch_prepare_pen(a, bcv.on() ? &v : nullptr, visc.mu, pen.args(), stream);
  else if (visc.on())  // variable viscosity (viscosity.cpp): the VISC forms only with a field
    launch_prepare_visc(a, bcv.on() ? &v : nullptr, visc.mu, stream);
  else if (bcv.on())  // prescribed boundary velocities (boundary_velocity.cpp): the BCV form only with a selection
    launch_prepare_bcv(a, v, stream);
  else
    launch_prepare(a, stream);
  check_launch("prepare");
  // commit d_p / grad_p (snapshot semantics): swap the scratch into the slot
  std::swap(S().dp, dp_scratch);
  std::swap(S().gp, gp_scratch);
  if (dist())  // assemble reads the neighbours' new d_p (and gradients for SOU/QUICK)
    halo(cell_plan, {{S().dp, 1}, {(float*)S().gp, 2}, {(float*)grad_u, 2}, {(float*)grad_v, 2}});
}

void Solver::assemble() {
  AssembleArgs a;
  a.N = N;
  a.ld = topo.ld;
  a.c = constants;
  a.fs = fs;
  a.vol = d_vol;
  a.st = S();
  a.u_old = ring[i_old].u;
  a.u_old_old = ring[i_old_old].u;
  a.flux_s = flux_s;
  a.grad_u = grad_u;
  a.grad_v = grad_v;
  a.srank_diag = d_sdrank;
  a.cslot_diag = d_tdrank8;
  a.cval_a = cval_a;
  a.cval_g = cval_g;
  a.cdiag2 = cdiag2;
  a.sval = sval;
  a.rhs = rhs;
  a.dinv_uv = dinv_uv;
  a.dinv_p = dinv_p;
  // Boussinesq buoyancy (scalar.cpp): the buoyant form only when a field drives
  // and g != 0; otherwise the plain kernel with the arguments it always had
  BuoyancyArgs b;
  const bool buoyant = scalars.buoyancy_args(b);
  const BcvArgs v = bcv.args();
  if (pen.on())  // volume penalisation: the PEN form of any of the eight
    launch_assemble_pen(a, buoyant ? &b : nullptr, bcv.on() ? &v : nullptr, visc.mu, pen.args(), stream);
  else if (visc.on())  // variable viscosity: the VISC form of any of the four
    launch_assemble_visc(a, buoyant ? &b : nullptr, bcv.on() ? &v : nullptr, visc.mu, stream);
  else if (bcv.on())  // prescribed boundary velocities: the BCV form of either
    launch_assemble_bcv(a, buoyant ? &b : nullptr, v, stream);
  else if (buoyant)
    launch_assemble_buoyant(a, b, stream);
  else
    launch_assemble(a, stream);
  check_launch("assemble");
  if (dist()) halo(cell_plan, {{dinv_uv, 1}});  // the Schur prediction reads neighbours' D_u^-1
}

// check_evolution (coupled_solver.rs:501-580), statistics on the GPU.  The
// stride bug (§0.1-12) makes index i read record i >> 2: a distributed rank
// first fetches the records [ev_a, ev_b) its indices read from their owners.
void Solver::check_evolution() {
  StateView var = S();
  uint64_t gbase = 0, rec0 = 0;
  if (dist()) {
    std::vector<Msg> msgs;
    StateView& cur = S();
    const uint64_t c0 = topo.c0, c1 = topo.c1;
    // owned records [lo, hi) to rank q, or those of rank q; one message per field, in field order
    auto add = [&](int q, bool send, uint64_t lo, uint64_t hi) {
      const size_t n = hi - lo, o = lo - (send ? c0 : ev_a);
      for_each_field(send ? cur : evrec, [&](float* base, int comps) {
        float* p = base + o * comps;
        const size_t bytes = n * comps * sizeof(float);
        msgs.push_back(send ? Msg{q, p, bytes, nullptr, 0} : Msg{q, nullptr, 0, p, bytes});
      });
    };
    for (int q = 0; q < R; ++q) {
      const uint64_t qa = starts[q] >> 2, qb = ((starts[q + 1] - 1) >> 2) + 1;  // q's record range
      // what q reads from me
      const uint64_t slo = std::max(qa, c0), shi = std::min(qb, c1);
      // what I read from q
      const uint64_t rlo = std::max(ev_a, starts[q]), rhi = std::min(ev_b, starts[q + 1]);
      if (q == rk) {
        if (rlo < rhi) {
          const size_t n = rhi - rlo, so = rlo - c0, ro = rlo - ev_a;
          for_each_field(evrec, cur, [&](float* to, const float* from, int comps) {
            CFD_HIP(hipMemcpyAsync(to + ro * comps, from + so * comps, n * comps * sizeof(float),
                                   hipMemcpyDeviceToDevice, stream));
          });
        }
        continue;
      }
      if (slo < shi) add(q, true, slo, shi);
      if (rlo < rhi) add(q, false, rlo, rhi);
    }
    comm->label = kCommStateHalo;
    comm->exchange(msgs, stream);
    var = evrec;
    gbase = topo.c0;
    rec0 = ev_a;
  }
  double tot[5];
  if (ref_red) {
    evolution_reference(tot);
  } else {
    launch_evolution_partial(S(), prev, have_prev ? 1 : 0, N, var, gbase, rec0, red.U, partial_d, pstride, stream);
    double* out5 = partial_d + 5 * (size_t)pstride;
    launch_evolution_final(combine(partial_d, 5), out5, stream);
    check_launch("check_evolution");
    CFD_HIP(hipMemcpyAsync(tot, out5, sizeof(tot), hipMemcpyDeviceToHost, stream));
  }
  copy_state(S(), prev, 0, N, stream);
  sync();
  const double nn = (double)NG;
  const double mean_u = tot[1] / nn, mean_v = tot[2] / nn;
  const double var_u = std::fmax(tot[3] / nn - mean_u * mean_u, 0.0);
  const double var_v = std::fmax(tot[4] / nn - mean_v * mean_v, 0.0);
  variance_history.push_back({var_u, var_v});
  if (variance_history.size() > 10) variance_history.erase(variance_history.begin());
  const double evo = have_prev ? std::sqrt(tot[0] / nn) : std::numeric_limits<double>::max();
  have_prev = true;
  if (evo < 1e-6) {
    if (var_u < 1e-10 && var_v < 1e-10) {
      info.degenerate_count++;
      info.steady_state_count = 0;
    } else {
      info.steady_state_count++;
      info.degenerate_count = 0;
    }
  } else {
    info.degenerate_count = 0;
    info.steady_state_count = 0;
  }
  if (info.degenerate_count > 10) {
    log("Solution is degenerate: Velocity field is uniform and not evolving. Variance U: %s, V: %s\n",
        e2(var_u).c_str(), e2(var_v).c_str());
    info.should_stop = 1;
  }
  if (info.steady_state_count > 10) {
    log("Steady state reached. Evolution diff: %s\n", e2(evo).c_str());
    info.should_stop = 1;
  }
}

void Solver::step() {  // coupled_solver.rs:33-499
  const Range range("cfd step");
  CFD_HIP(hipSetDevice(device));
  // opt-in deviation from the frozen hierarchy
  if (cfg.amg_rebuild_interval > 0 && amg_built && amg_age >= (uint32_t)cfg.amg_rebuild_interval) {
    // numeric re-setup over the kept structure when the device setup built it
    // (CFD_AMG_SETUP=rebuild: full rebuild; both give the same hierarchy)
    const char* se = knob(Knob::AmgSetup);  // "rebuild": a full setup instead of the refresh
    if (amg_setup_path == 2 && !amg_refresh.empty() && !(se && std::strcmp(se, "rebuild") == 0))
      amg_refresh_pending = true;
    else
      drop_amg();
  }
  rotate();
  constants.component = 0;
  last_step_dt = constants.dt;  // host only: cfd_scalar_advance(dt <= 0) advances by the step's dt
  const int fault_rank = debug_fault_after_prepare;  // test hook, one step only
  debug_fault_after_prepare = -1;
  if (dist()) halo_state(true);  // the rotated slot's ghosts (last written 3 steps ago)
  if (visc.has_model()) visc.evaluate(view(nullptr));  // the step's viscosity, from the velocity it starts from
  prepare();
  if (fault_rank == rk) throw std::runtime_error("injected fault after prepare");
  const bool fixed = cfg.fixed_outer > 0;
  const int max_iters = fixed ? cfg.fixed_outer : std::max(cfg.n_outer_correctors, 10);
  const double tol_u = 1e-5, tol_p = 1e-4;
  double prev_u = std::numeric_limits<double>::max(), prev_p = std::numeric_limits<double>::max();
  outer.reset();  // per step (coupled_solver.rs:119-121)
  info.total_linear_iterations = 0;
  for (int iter = 0; iter < max_iters; ++iter) {
    const Range outer_range("picard iteration");
    log("Coupled Iteration: %d\n", iter + 1);
    if (iter > 0 || constants.scheme != 0) prepare();
    assemble();
    const cfd_linear_stats ls = solve();
    log("Coupled linear solve: %u iterations, residual %s, converged=%s\n", ls.iterations, e2(ls.residual).c_str(),
        tf(ls.converged));
    info.stats_p = ls;
    info.total_linear_iterations += ls.iterations;
    if (std::isnan(ls.residual)) throw std::domain_error("Coupled Linear Solver Diverged: NaN detected in linear residual");
    // the final max-diff pair also lands in a pinned host slot: the lagged read
    // below needs no copy launch.  Either slot will do (iteration 0 writes one
    // and never submits it): writer and reader take it from this one call.
    const int wslot = outer.write_slot();
    uint32_t* host_slot = reinterpret_cast<uint32_t*>(d_pin + kPinOuter + 2 * wslot);
    launch_update_fields(N, constants.alpha_u, constants.alpha_p, x, S().u, S().p, blockmax, maxbits,
                         dist() ? nullptr : host_slot, stream);
    check_launch("update_fields");
    if (dist()) {
      halo_state(false);  // the next prepare reads neighbours' u, p
      timed_gather(kCommReduceGather, 2 * sizeof(uint32_t),
                   [&] { comm->allgather(maxbits, mx_gather, 2 * sizeof(uint32_t), stream); });
      launch_max_combine(mx_gather, R, maxbits, host_slot, stream);
    }
    if (iter == 0) {
      info.outer_residual_u = std::numeric_limits<float>::max();
      info.outer_residual_p = std::numeric_limits<float>::max();
      info.outer_iterations = 1;
      continue;
    }
    // async max-diff read (coupled_solver.rs:396-479) under the lag model
    outer.submit(wslot, stream, cfg.convergence_lag);
    if (!outer.have()) continue;
    const float cu = outer.last(0), cp = outer.last(1);
    const double du = cu, dp = cp;
    if (std::isnan(du) || std::isnan(dp)) throw std::domain_error("Coupled Solver Diverged: NaN detected in outer residuals");
    info.outer_residual_u = cu;
    info.outer_residual_p = cp;
    info.outer_iterations = iter + 1;
    log("Coupled Residuals - U: %s, P: %s\n", e2(du).c_str(), e2(dp).c_str());
    if (!fixed) {
      if (du < tol_u && dp < tol_p) {
        log("Coupled Solver Converged in %d iterations\n", iter + 1);
        break;
      }
      const double rel_u = (std::isfinite(prev_u) && std::fabs(prev_u) > 1e-14) ? std::fabs((du - prev_u) / prev_u)
                                                                                : std::numeric_limits<double>::infinity();
      const double rel_p = (std::isfinite(prev_p) && std::fabs(prev_p) > 1e-14) ? std::fabs((dp - prev_p) / prev_p)
                                                                                : std::numeric_limits<double>::infinity();
      if (rel_u < 1e-2 && rel_p < 1e-2 && iter > 2) {
        log("Coupled solver stagnated at iter %d: U=%s, P=%s\n", iter + 1, e2(du).c_str(), e2(dp).c_str());
        break;
      }
    }
    prev_u = du;
    prev_p = dp;
  }
  constants.time += constants.dt;
  if (amg_built) ++amg_age;
  check_evolution();
}

}  // namespace cfd2
