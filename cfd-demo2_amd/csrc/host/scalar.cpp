// Passive scalar transport (include/cfd2_amd.h, the last section; kernels.hpp
// "scalar.hip"): per advance and field one face-slot assembly from flux_s as
// the last k_prepare left it, then Jacobi sweeps in batches of check_interval,
// the host reading the last sweep's delta after each batch.  A field on method
// 1 runs BiCGStab between the two and starts the sweeps from its answer.  A
// field on scheme 1 takes its right-hand side from the gradient pass and the
// limited assembly instead; everything after the assembly is the same.  A field
// with a wall condition or a source (kernels.hpp ScalarBC) runs the boundary-
// condition forms of those passes; a field without runs the plain ones.
#include <cmath>
#include <cstring>

#include "scalars.hpp"

namespace cfd2 {

// the words of the calls that refuse a distributed handle
static void one_gpu(const FlowView& flow, const char* what) {
  if (flow.dist)
    throw std::invalid_argument(std::string("passive scalars run on one GPU only: no ") + what + " on a distributed handle");
}

void Scalars::enable(const FlowView& flow, int count, const cfd_scalar_config& c) {
  if (count < 0 || count > 4) throw std::invalid_argument("scalar field count must be 0..4");
  if (flow.dist)
    throw std::invalid_argument("passive scalars run on one GPU only: a distributed handle has no halo exchange per "
                                "Jacobi sweep");
  if (count > 0) {
    if (!(c.tol >= 0.0f)) throw std::invalid_argument("scalar config: tol must be >= 0");
    if (c.check_interval < 1) throw std::invalid_argument("scalar config: check_interval must be >= 1");
    if (c.max_sweeps < 1) throw std::invalid_argument("scalar config: max_sweeps must be >= 1");
  }
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();
  arena.release();
  ++gen;
  s = {};
  if (count == 0) return;
  const size_t ld = flow.ld;
  const size_t nbm = std::max<size_t>(scalar_sweep_blocks(flow.N), 2 * (size_t)red_blocks(flow.N));
  auto field = [&] {
    float* p = arena.alloc<float>(ld);
    CFD_HIP(hipMemsetAsync(p, 0, ld * sizeof(float), flow.stream));
    return p;
  };
  for (int f = 0; f < count; ++f) s.field[f].phi = field();
  s.alt = field();
  s.coef = arena.alloc<float>((size_t)flow.fs.wf * ld);
  s.diag = arena.alloc<float>(ld);
  s.b = arena.alloc<float>(ld);
  s.blockmax = arena.alloc<uint32_t>(nbm);
  s.res = arena.alloc<ScalarResults>(1);
  s.partial = arena.alloc<double>(flow.sums.pstride);
  flow.sync();
  cfg = c;
  cfg.reserved = 0;
  s.count = count;
}

void Scalars::set_params(const FlowView&, int field, const cfd_scalar_params& p) {
  check(field);
  if (!(p.diffusivity >= 0.0f)) throw std::invalid_argument("scalar diffusivity must be >= 0");
  s.field[field].par = p;
}

void Scalars::set(const FlowView& flow, int field, const double* phi) {
  check(field);
  CFD_HIP(hipSetDevice(flow.device));
  std::vector<float> h(flow.N);
  for (uint32_t i = 0; i < flow.N; ++i) h[i] = (float)phi[i];
  CFD_HIP(hipMemcpyAsync(s.field[field].phi, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, flow.stream));
  flow.sync();
}

void Scalars::get(const FlowView& flow, int field, double* phi) {
  check(field);
  CFD_HIP(hipSetDevice(flow.device));
  std::vector<float> h(flow.N);
  CFD_HIP(hipMemcpyAsync(h.data(), s.field[field].phi, h.size() * sizeof(float), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  for (uint32_t i = 0; i < flow.N; ++i) phi[i] = h[i];
}

void Scalars::advance(const FlowView& flow, float dt) {
  if (s.count == 0) throw std::invalid_argument("passive scalars are not enabled (cfd_scalars_enable)");
  if (!(dt > 0.0f)) {
    if (!(flow.last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_scalar_advance: dt <= 0 asks for the dt of the last cfd_step, and there was none");
    dt = flow.last_step_dt;
  }
  const Range range("scalar advance");
  CFD_HIP(hipSetDevice(flow.device));
  for (int fi = 0; fi < s.count; ++fi) {
    ScalarField& f = s.field[fi];
    ScalarAssembleArgs A{};
    A.N = flow.N;
    A.ld = flow.ld;
    A.fs = flow.fs;
    A.vol = flow.vol;
    A.flux_s = flow.flux_s;
    A.phi_old = f.phi;
    A.density = flow.constants.density;
    A.dt = dt;
    A.diffusivity = f.par.diffusivity;
    A.inlet_value = f.par.inlet_value;
    A.coef = s.coef;
    A.diag = s.diag;
    A.b = s.b;
    f.scheme_used = f.scheme;
    f.clamped = 0;
    const bool bc = f.wall_on() || f.source_on();
    const ScalarBC B{f.sel, f.wall_on() ? f.wall.kind : 0, f.wall.value, f.source_on() ? f.source.rate : 0.0f};
    if (f.scheme == 1) {
      // the gradient of phi_old first, every cell before any is read; then the
      // assembly with the limited right-hand side.  The count lands in
      // f.clamped with the first read of the solve below.
      if (B.kind == 1)
        launch_scalar_grad_bc(ScalarGradArgs(A, s.hr_grad), B, flow.stream);
      else
        launch_scalar_grad(ScalarGradArgs(A, s.hr_grad), flow.stream);
      CFD_HIP(hipMemsetAsync(s.hr_count + fi, 0, sizeof(uint32_t), flow.stream));
      if (bc)
        launch_scalar_assemble_limited_bc(ScalarLimitedArgs{A, s.hr_grad, s.hr_count + fi}, B, flow.stream);
      else
        launch_scalar_assemble_limited(ScalarLimitedArgs{A, s.hr_grad, s.hr_count + fi}, flow.stream);
      flow.check_launch("scalar limited assemble");
      CFD_HIP(hipMemcpyAsync(&f.clamped, s.hr_count + fi, sizeof(uint32_t), hipMemcpyDeviceToHost, flow.stream));
    } else {
      if (bc)
        launch_scalar_assemble_bc(A, B, flow.stream);
      else
        launch_scalar_assemble(A, flow.stream);
      flow.check_launch("scalar assemble");
    }
    f.sweeps = 0;
    f.converged = 0;
    f.dt_used = dt;
    f.kstats = cfd_scalar_solver_stats{};
    f.kstats.method = f.solver.method;
    if (f.solver.method == 1) krylov(flow, f);
    polish(flow, fi, f);
    if (f.solver.method == 1) f.kstats.polish_sweeps = f.sweeps;
  }
}

ScalarSystem Scalars::system(const FlowView& flow) const {
  return ScalarSystem{flow.N, (uint32_t)flow.ld, flow.fs.other, flow.fs.nface, s.coef, s.diag, s.b};
}

// The Jacobi loop from f.phi, in batches of check_interval sweeps.
void Scalars::polish(const FlowView& flow, int fi, ScalarField& f) {
  const uint32_t ci = (uint32_t)cfg.check_interval;
  const uint32_t max_sweeps = ((uint32_t)cfg.max_sweeps + ci - 1) / ci * ci;
  ScalarSweepArgs W{};
  W.sys = system(flow);
  W.blockmax = s.blockmax;
  uint32_t bits = 0;
  while (f.sweeps < max_sweeps) {
    for (uint32_t k = 0; k < ci; ++k) {  // phi^0 = phi_old; b holds a_t * phi_old, so its buffer is free to swap
      W.phi_in = f.phi;
      W.phi_out = s.alt;
      launch_scalar_sweep(W, k + 1 == ci ? &s.res->delta : nullptr, flow.stream);
      std::swap(f.phi, s.alt);
    }
    flow.check_launch("scalar sweep");
    CFD_HIP(hipMemcpyAsync(&bits, &s.res->delta, sizeof(bits), hipMemcpyDeviceToHost, flow.stream));
    flow.sync();
    f.sweeps += ci;
    std::memcpy(&f.last_delta, &bits, 4);
    if (!std::isfinite(f.last_delta))
      throw std::domain_error("scalar field " + std::to_string(fi) + " diverged: non-finite Jacobi update after " +
                              std::to_string(f.sweeps) + " sweeps");
    if (f.last_delta <= cfg.tol) {
      f.converged = 1;
      break;
    }
  }
}

// BiCGStab on the Jacobi-scaled system (include/cfd2_amd.h "Arithmetic of
// method 1"), x in place in f.phi: iterations in batches of the field's
// check_interval, one read of the four status words per batch.  Every kernel
// returns at once after the device recorded a stop, so the batch size changes
// nothing but the number of reads.
void Scalars::krylov(const FlowView& flow, ScalarField& f) {
  ScalarKrylovArgs K{};
  K.sys = system(flow);
  K.x = f.phi;
  K.rh = s.kr_vec[0];
  K.r = s.kr_vec[1];
  K.p = s.kr_vec[2];
  K.v = s.kr_vec[3];
  K.s = s.kr_vec[4];
  K.t = s.kr_vec[5];
  K.out = flow.sums.out(s.kr_partial);
  K.blockmax = s.blockmax;
  K.state = s.kr_state;
  K.red = flow.sums.src(s.kr_partial, 2);
  K.tol = cfg.tol;
  uint32_t st[4] = {0, 0, 0, 0};
  auto read = [&](const char* where) {
    flow.check_launch(where);
    CFD_HIP(hipMemcpyAsync(st, s.kr_state->st, sizeof(st), hipMemcpyDeviceToHost, flow.stream));
    flow.sync();
  };
  launch_scalar_krylov_start(K, flow.stream);
  read("scalar krylov start");
  const uint32_t cap = (uint32_t)f.solver.max_iters, ci = (uint32_t)f.solver.check_interval;
  uint32_t k = 0;
  while (!st[kKryDone] && k < cap) {
    const uint32_t end = std::min(cap, k + ci);
    while (k < end) launch_scalar_krylov_iteration(K, ++k, cap, flow.stream);
    read("scalar krylov iteration");
  }
  f.kstats.iterations = st[kKryDone] ? (int32_t)st[kKryIter] : (int32_t)cap;
  f.kstats.stop_reason = st[kKryDone] ? (int32_t)st[kKryReason] : 3;
  std::memcpy(&f.kstats.krylov_residual, &st[kKryRes], 4);
}

void Scalars::set_solver(const FlowView& flow, int field, const cfd_scalar_solver& c) {
  one_gpu(flow, "scalar solver");
  check(field);
  if (c.method != 0 && c.method != 1) throw std::invalid_argument("scalar solver: method must be 0 (Jacobi) or 1 (BiCGStab)");
  if (c.max_iters < 1) throw std::invalid_argument("scalar solver: max_iters must be >= 1");
  if (c.check_interval < 1) throw std::invalid_argument("scalar solver: check_interval must be >= 1");
  if (c.method == 1 && !s.kr_state) {
    CFD_HIP(hipSetDevice(flow.device));
    for (float*& v : s.kr_vec) v = arena.alloc<float>(flow.ld);
    s.kr_partial = arena.alloc<double>(2 * (size_t)flow.sums.pstride);
    s.kr_state = arena.alloc<ScalarKrylovState>(1);
  }
  s.field[field].solver = c;
  s.field[field].solver.reserved = 0;
}

void Scalars::solver_stats(const FlowView& flow, int field, cfd_scalar_solver_stats* out) const {
  one_gpu(flow, "scalar solver");
  check(field);
  *out = s.field[field].kstats;
}

void Scalars::set_scheme(const FlowView& flow, int field, const cfd_scalar_scheme& c) {
  one_gpu(flow, "scalar scheme");
  check(field);
  if (c.scheme != 0 && c.scheme != 1)
    throw std::invalid_argument("scalar scheme: scheme must be 0 (upwind) or 1 (limited linear)");
  if (c.scheme == 1 && !s.hr_grad) {
    if (flow.fs.wf > 32) throw std::invalid_argument("scalar scheme 1 keeps a cell's inlet slots in 32 bits: more than 32 faces per cell");
    CFD_HIP(hipSetDevice(flow.device));
    s.hr_grad = arena.alloc<float2>(flow.ld);
    s.hr_count = arena.alloc<uint32_t>(4);
    CFD_HIP(hipMemsetAsync(s.hr_count, 0, 4 * sizeof(uint32_t), flow.stream));
  }
  s.field[field].scheme = c.scheme;
}

void Scalars::scheme_stats(const FlowView& flow, int field, cfd_scalar_scheme_stats* out) const {
  one_gpu(flow, "scalar scheme");
  check(field);
  std::memset(out, 0, sizeof(*out));
  out->scheme = s.field[field].scheme_used;
  out->clamped_cells = s.field[field].clamped;
}

// The selection image of one field from its wall box and its source box: bit k
// < 31 of word i = slot k of cell i is a selected wall face (kind 1 or 2 only),
// bit 31 = cell i is a source cell (rate != 0 only).  Allocated at the first
// selection that sets a bit; a field without one keeps the plain kernels.
void Scalars::select(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
                     const std::vector<double>& cy, ScalarField& f) {
  if (!f.wall_on() && !f.source_on()) return;
  std::vector<uint32_t> img(flow.N, 0u);
  if (f.wall_on()) {
    const cfd_scalar_wall& w = f.wall;
    for (const WallFace& wfc : wall)
      if (wfc.cx >= w.x0 && wfc.cx <= w.x1 && wfc.cy >= w.y0 && wfc.cy <= w.y1) img[wfc.cell] |= 1u << wfc.slot;
  }
  if (f.source_on()) {
    const cfd_scalar_source& q = f.source;
    for (uint32_t i = 0; i < flow.N; ++i)
      if (cx[i] >= q.x0 && cx[i] <= q.x1 && cy[i] >= q.y0 && cy[i] <= q.y1) img[i] |= 1u << 31;
  }
  CFD_HIP(hipSetDevice(flow.device));
  if (!f.sel) f.sel = arena.alloc<uint32_t>(flow.N);
  CFD_HIP(hipMemcpyAsync(f.sel, img.data(), (size_t)flow.N * sizeof(uint32_t), hipMemcpyHostToDevice, flow.stream));
  flow.sync();
}

uint32_t Scalars::set_wall(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
                           const std::vector<double>& cy, int field, const cfd_scalar_wall& c) {
  one_gpu(flow, "scalar wall");
  check(field);
  if (c.kind < 0 || c.kind > 2)
    throw std::invalid_argument("scalar wall: kind must be 0 (adiabatic), 1 (fixed value) or 2 (fixed flux)");
  if (!std::isfinite(c.value)) throw std::invalid_argument("scalar wall: value must be finite");
  uint32_t count = 0;
  if (!(c.x1 < c.x0))
    for (const WallFace& wfc : wall) {
      if (!(wfc.cx >= c.x0 && wfc.cx <= c.x1 && wfc.cy >= c.y0 && wfc.cy <= c.y1)) continue;
      if (c.kind != 0 && wfc.slot >= 31)
        throw std::invalid_argument("scalar wall keeps a cell's selected wall slots in 31 bits: wall face at slot 31 or "
                                    "above of its cell");
      ++count;
    }
  ScalarField& f = s.field[field];
  f.wall = c;
  f.wall_n = count;
  ++gen;
  select(flow, wall, cx, cy, f);
  return count;
}

uint32_t Scalars::set_source(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
                             const std::vector<double>& cy, int field, const cfd_scalar_source& c) {
  one_gpu(flow, "scalar source");
  check(field);
  if (!std::isfinite(c.rate)) throw std::invalid_argument("scalar source: rate must be finite");
  uint32_t count = 0;
  if (!(c.x1 < c.x0))
    for (uint32_t i = 0; i < flow.N; ++i)
      if (cx[i] >= c.x0 && cx[i] <= c.x1 && cy[i] >= c.y0 && cy[i] <= c.y1) ++count;
  ScalarField& f = s.field[field];
  f.source = c;
  f.source_n = count;
  select(flow, wall, cx, cy, f);
  return count;
}

SurfaceField Scalars::surface_field(int fi, float density) const {
  SurfaceField d{};
  if (fi >= s.count) return d;
  const ScalarField& f = s.field[fi];
  d.phi = f.phi;
  d.sel = f.wall_on() ? f.sel : nullptr;  // wall_flux's own condition
  d.rd = density * f.par.diffusivity;
  d.kind = f.wall.kind;
  d.value = f.wall.value;
  return d;
}

// Read-only on the current field, with the current density and diffusivity; a
// field without selected faces launches nothing.
void Scalars::wall_flux(const FlowView& flow, int field, cfd_scalar_wall_flux* out) {
  one_gpu(flow, "scalar wall flux");
  check(field);
  const ScalarField& f = s.field[field];
  std::memset(out, 0, sizeof(*out));
  out->faces = f.wall_n;
  out->kind = f.wall.kind;
  if (!f.wall_on()) return;
  CFD_HIP(hipSetDevice(flow.device));
  ScalarWallFluxArgs a{};
  a.N = flow.N;
  a.area = flow.fs.area;
  a.dist_e = flow.fs.dist_e;
  a.sel = f.sel;
  a.phi = f.phi;
  a.rd = flow.constants.density * f.par.diffusivity;
  a.kind = f.wall.kind;
  a.value = f.wall.value;
  a.out = flow.sums.buf(s.wf_sums, kWallFluxSums, arena);
  launch_scalar_wall_flux(a, flow.stream);
  double h[kWallFluxSums];
  flow.sum_read(s.wf_sums, kWallFluxSums, h, "scalar wall flux");
  out->flux = h[0];
  out->area = h[1];
  out->phi_area = h[2];
}

// ---- Boussinesq buoyancy ----
void Scalars::set_buoyancy(const FlowView& flow, int field, float beta, float ref) {
  one_gpu(flow, "buoyancy");
  check(field);
  if (!std::isfinite(beta) || !std::isfinite(ref)) throw std::invalid_argument("scalar buoyancy: beta and ref must be finite");
  s.field[field].beta = beta;
  s.field[field].bref = ref;
}

void Scalars::set_gravity(const FlowView& flow, float gx, float gy) {
  one_gpu(flow, "gravity");
  if (!std::isfinite(gx) || !std::isfinite(gy)) throw std::invalid_argument("gravity: g_x and g_y must be finite");
  gravity[0] = gx;
  gravity[1] = gy;
}

// The field pointers are read here, at launch time: f.phi swaps with s.alt
// during an advance.
bool Scalars::buoyancy_args(BuoyancyArgs& b) const {
  b = BuoyancyArgs{};
  for (int fi = 0; fi < s.count; ++fi) {
    const ScalarField& f = s.field[fi];
    if (f.beta != 0.0f) b.f[b.n++] = BuoyancyField{f.phi, f.beta, f.bref};
  }
  b.gx = gravity[0];
  b.gy = gravity[1];
  return b.n > 0 && (b.gx != 0.0f || b.gy != 0.0f);
}

void Scalars::buoyancy_get(const FlowView&, cfd_buoyancy* out) const {
  std::memset(out, 0, sizeof(*out));
  out->gx = gravity[0];
  out->gy = gravity[1];
  out->fields = s.count;
  for (int fi = 0; fi < s.count; ++fi) {
    out->beta[fi] = s.field[fi].beta;
    out->ref[fi] = s.field[fi].bref;
  }
  BuoyancyArgs b;
  out->active = buoyancy_args(b) ? 1 : 0;
}

// Read-only on the current fields, with the current density; launches nothing
// unless the assembly would take its buoyant form.
void Scalars::buoyancy_force(const FlowView& flow, cfd_buoyancy_force* out) {
  one_gpu(flow, "buoyancy force");
  if (s.count == 0) throw std::invalid_argument("passive scalars are not enabled (cfd_scalars_enable)");
  std::memset(out, 0, sizeof(*out));
  BuoyancyForceArgs a{};
  const bool on = buoyancy_args(a.b);
  out->fields = (uint32_t)a.b.n;
  if (!on) return;
  CFD_HIP(hipSetDevice(flow.device));
  a.N = flow.N;
  a.vol = flow.vol;
  a.density = flow.constants.density;
  a.out = flow.sums.buf(s.bf_sums, kBuoyancySums, arena);
  launch_buoyancy_force(a, flow.stream);
  double h[kBuoyancySums];
  flow.sum_read(s.bf_sums, kBuoyancySums, h, "buoyancy force");
  out->force[0] = h[0];
  out->force[1] = h[1];
}

void Scalars::stats(const FlowView& flow, int field, cfd_scalar_stats* out) {
  check(field);
  CFD_HIP(hipSetDevice(flow.device));
  const ScalarField& f = s.field[field];
  ScalarStatsArgs a{};
  a.N = flow.N;
  a.vol = flow.vol;
  a.phi = f.phi;
  a.out = flow.sums.out(s.partial);
  a.blockmm = s.blockmax;
  launch_scalar_stats(a, s.res, flow.stream);
  launch_evolution_final(flow.sums.src(s.partial, 1), &s.res->integral, flow.stream);
  flow.check_launch("scalar stats");
  ScalarResults h;
  CFD_HIP(hipMemcpyAsync(&h, s.res, sizeof(h), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  const uint32_t bmin = scalar_key_value(h.kmin), bmax = scalar_key_value(h.kmax);
  float vmin, vmax;
  std::memcpy(&vmin, &bmin, 4);
  std::memcpy(&vmax, &bmax, 4);
  std::memset(out, 0, sizeof(*out));
  out->sweeps = f.sweeps;
  out->converged = f.converged;
  out->last_delta = f.last_delta;
  out->dt_used = f.dt_used;
  out->min = vmin;
  out->max = vmax;
  out->integral = h.integral;
}

}  // namespace cfd2
