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

#include "solver_impl.hpp"

namespace cfd2 {

void Solver::scalars_enable(int count, const cfd_scalar_config& c) {
  if (count < 0 || count > 4) throw std::invalid_argument("scalar field count must be 0..4");
  if (dist())
    throw std::invalid_argument("passive scalars run on one GPU only: a distributed handle has no halo exchange per "
                                "Jacobi sweep");
  if (count > 0) {
    if (!(c.tol >= 0.0f)) throw std::invalid_argument("scalar config: tol must be >= 0");
    if (c.check_interval < 1) throw std::invalid_argument("scalar config: check_interval must be >= 1");
    if (c.max_sweeps < 1) throw std::invalid_argument("scalar config: max_sweeps must be >= 1");
  }
  CFD_HIP(hipSetDevice(device));
  sync();
  sc_arena.release();
  ++surface_gen;  // a surface re-derives its channels and resets its statistics (surface.cpp)
  sc_count = 0;
  sc_alt = sc_coef = sc_diag = sc_b = nullptr;
  sc_blockmax = nullptr;
  sc_res = nullptr;
  sc_partial = nullptr;
  for (float*& v : kr_vec) v = nullptr;
  kr_partial = nullptr;
  kr_state = nullptr;
  hr_grad = nullptr;
  hr_count = nullptr;
  wf_sums = bf_sums = SumBuf{};
  for (ScalarField& f : sc_field) f = ScalarField{};  // every beta back to 0: the step is the plain one again
  if (count == 0) return;
  const size_t ld = topo.ld;
  const size_t nbm = std::max<size_t>(scalar_sweep_blocks(N), 2 * (size_t)red_blocks(N));
  auto field = [&] {
    float* p = sc_arena.alloc<float>(ld);
    CFD_HIP(hipMemsetAsync(p, 0, ld * sizeof(float), stream));
    return p;
  };
  for (int f = 0; f < count; ++f) sc_field[f].phi = field();
  sc_alt = field();
  sc_coef = sc_arena.alloc<float>((size_t)topo.wf * ld);
  sc_diag = sc_arena.alloc<float>(ld);
  sc_b = sc_arena.alloc<float>(ld);
  sc_blockmax = sc_arena.alloc<uint32_t>(nbm);
  sc_res = sc_arena.alloc<ScalarResults>(1);
  sc_partial = sc_arena.alloc<double>(pstride);
  sync();
  sc_cfg = c;
  sc_cfg.reserved = 0;
  sc_count = count;
}

void Solver::scalar_check(int field) const { scalar_index_check(sc_count, field); }

void Solver::set_scalar(int field, const double* phi) {
  scalar_check(field);
  CFD_HIP(hipSetDevice(device));
  std::vector<float> h(N);
  for (uint32_t i = 0; i < N; ++i) h[i] = (float)phi[i];
  CFD_HIP(hipMemcpyAsync(sc_field[field].phi, h.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice, stream));
  sync();
}

void Solver::get_scalar(int field, double* phi) {
  scalar_check(field);
  CFD_HIP(hipSetDevice(device));
  std::vector<float> h(N);
  CFD_HIP(hipMemcpyAsync(h.data(), sc_field[field].phi, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) phi[i] = h[i];
}

void Solver::scalar_advance(float dt) {
  if (sc_count == 0) throw std::invalid_argument("passive scalars are not enabled (cfd_scalars_enable)");
  if (!(dt > 0.0f)) {
    if (!(last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_scalar_advance: dt <= 0 asks for the dt of the last cfd_step, and there was none");
    dt = last_step_dt;
  }
  const Range range("scalar advance");
  CFD_HIP(hipSetDevice(device));
  for (int fi = 0; fi < sc_count; ++fi) {
    ScalarField& f = sc_field[fi];
    ScalarAssembleArgs A{};
    A.N = N;
    A.ld = topo.ld;
    A.fs = fs;
    A.vol = d_vol;
    A.flux_s = flux_s;
    A.phi_old = f.phi;
    A.density = constants.density;
    A.dt = dt;
    A.diffusivity = f.par.diffusivity;
    A.inlet_value = f.par.inlet_value;
    A.coef = sc_coef;
    A.diag = sc_diag;
    A.b = sc_b;
    f.scheme_used = f.scheme;
    f.clamped = 0;
    const bool bc = f.wall_on() || f.source_on();
    const ScalarBC B{f.sel, f.wall_on() ? f.wall.kind : 0, f.wall.value, f.source_on() ? f.source.rate : 0.0f};
    if (f.scheme == 1) {
      // the gradient of phi_old first, every cell before any is read; then the
      // assembly with the limited right-hand side.  The count lands in
      // f.clamped with the first read of the solve below.
      if (B.kind == 1)
        launch_scalar_grad_bc(ScalarGradArgs(A, hr_grad), B, stream);
      else
        launch_scalar_grad(ScalarGradArgs(A, hr_grad), stream);
      CFD_HIP(hipMemsetAsync(hr_count + fi, 0, sizeof(uint32_t), stream));
      if (bc)
        launch_scalar_assemble_limited_bc(ScalarLimitedArgs{A, hr_grad, hr_count + fi}, B, stream);
      else
        launch_scalar_assemble_limited(ScalarLimitedArgs{A, hr_grad, hr_count + fi}, stream);
      check_launch("scalar limited assemble");
      CFD_HIP(hipMemcpyAsync(&f.clamped, hr_count + fi, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    } else {
      if (bc)
        launch_scalar_assemble_bc(A, B, stream);
      else
        launch_scalar_assemble(A, stream);
      check_launch("scalar assemble");
    }
    f.sweeps = 0;
    f.converged = 0;
    f.dt_used = dt;
    f.kstats = cfd_scalar_solver_stats{};
    f.kstats.method = f.solver.method;
    if (f.solver.method == 1) scalar_krylov(f);
    scalar_polish(fi, f);
    if (f.solver.method == 1) f.kstats.polish_sweeps = f.sweeps;
  }
}

ScalarSystem Solver::scalar_system() const {
  return ScalarSystem{N, (uint32_t)topo.ld, fs.other, fs.nface, sc_coef, sc_diag, sc_b};
}

// The Jacobi loop from f.phi, in batches of check_interval sweeps.
void Solver::scalar_polish(int fi, ScalarField& f) {
  const uint32_t ci = (uint32_t)sc_cfg.check_interval;
  const uint32_t max_sweeps = ((uint32_t)sc_cfg.max_sweeps + ci - 1) / ci * ci;
  ScalarSweepArgs W{};
  W.sys = scalar_system();
  W.blockmax = sc_blockmax;
  uint32_t bits = 0;
  while (f.sweeps < max_sweeps) {
    for (uint32_t k = 0; k < ci; ++k) {  // phi^0 = phi_old; b holds a_t * phi_old, so its buffer is free to swap
      W.phi_in = f.phi;
      W.phi_out = sc_alt;
      launch_scalar_sweep(W, k + 1 == ci ? &sc_res->delta : nullptr, stream);
      std::swap(f.phi, sc_alt);
    }
    check_launch("scalar sweep");
    CFD_HIP(hipMemcpyAsync(&bits, &sc_res->delta, sizeof(bits), hipMemcpyDeviceToHost, stream));
    sync();
    f.sweeps += ci;
    std::memcpy(&f.last_delta, &bits, 4);
    if (!std::isfinite(f.last_delta))
      throw std::domain_error("scalar field " + std::to_string(fi) + " diverged: non-finite Jacobi update after " +
                              std::to_string(f.sweeps) + " sweeps");
    if (f.last_delta <= sc_cfg.tol) {
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
void Solver::scalar_krylov(ScalarField& f) {
  ScalarKrylovArgs K{};
  K.sys = scalar_system();
  K.x = f.phi;
  K.rh = kr_vec[0];
  K.r = kr_vec[1];
  K.p = kr_vec[2];
  K.v = kr_vec[3];
  K.s = kr_vec[4];
  K.t = kr_vec[5];
  K.out = sum_out(kr_partial);
  K.blockmax = sc_blockmax;
  K.state = kr_state;
  K.red = combine(kr_partial, 2);
  K.tol = sc_cfg.tol;
  uint32_t st[4] = {0, 0, 0, 0};
  auto read = [&](const char* where) {
    check_launch(where);
    CFD_HIP(hipMemcpyAsync(st, kr_state->st, sizeof(st), hipMemcpyDeviceToHost, stream));
    sync();
  };
  launch_scalar_krylov_start(K, stream);
  read("scalar krylov start");
  const uint32_t cap = (uint32_t)f.solver.max_iters, ci = (uint32_t)f.solver.check_interval;
  uint32_t k = 0;
  while (!st[kKryDone] && k < cap) {
    const uint32_t end = std::min(cap, k + ci);
    while (k < end) launch_scalar_krylov_iteration(K, ++k, cap, stream);
    read("scalar krylov iteration");
  }
  f.kstats.iterations = st[kKryDone] ? (int32_t)st[kKryIter] : (int32_t)cap;
  f.kstats.stop_reason = st[kKryDone] ? (int32_t)st[kKryReason] : 3;
  std::memcpy(&f.kstats.krylov_residual, &st[kKryRes], 4);
}

void Solver::set_scalar_solver(int field, const cfd_scalar_solver& c) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar solver on a distributed handle");
  scalar_check(field);
  if (c.method != 0 && c.method != 1) throw std::invalid_argument("scalar solver: method must be 0 (Jacobi) or 1 (BiCGStab)");
  if (c.max_iters < 1) throw std::invalid_argument("scalar solver: max_iters must be >= 1");
  if (c.check_interval < 1) throw std::invalid_argument("scalar solver: check_interval must be >= 1");
  if (c.method == 1 && !kr_state) {
    CFD_HIP(hipSetDevice(device));
    for (float*& v : kr_vec) v = sc_arena.alloc<float>(topo.ld);
    kr_partial = sc_arena.alloc<double>(2 * (size_t)pstride);
    kr_state = sc_arena.alloc<ScalarKrylovState>(1);
  }
  sc_field[field].solver = c;
  sc_field[field].solver.reserved = 0;
}

void Solver::set_scalar_scheme(int field, const cfd_scalar_scheme& c) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar scheme on a distributed handle");
  scalar_check(field);
  if (c.scheme != 0 && c.scheme != 1)
    throw std::invalid_argument("scalar scheme: scheme must be 0 (upwind) or 1 (limited linear)");
  if (c.scheme == 1 && !hr_grad) {
    if (topo.wf > 32) throw std::invalid_argument("scalar scheme 1 keeps a cell's inlet slots in 32 bits: more than 32 faces per cell");
    CFD_HIP(hipSetDevice(device));
    hr_grad = sc_arena.alloc<float2>(topo.ld);
    hr_count = sc_arena.alloc<uint32_t>(4);
    CFD_HIP(hipMemsetAsync(hr_count, 0, 4 * sizeof(uint32_t), stream));
  }
  sc_field[field].scheme = c.scheme;
}

void Solver::scalar_scheme_stats(int field, cfd_scalar_scheme_stats* out) const {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar scheme on a distributed handle");
  scalar_check(field);
  std::memset(out, 0, sizeof(*out));
  out->scheme = sc_field[field].scheme_used;
  out->clamped_cells = sc_field[field].clamped;
}

// The selection image of one field from its wall box and its source box: bit k
// < 31 of word i = slot k of cell i is a selected wall face (kind 1 or 2 only),
// bit 31 = cell i is a source cell (rate != 0 only).  Allocated at the first
// selection that sets a bit; a field without one keeps the plain kernels.
void Solver::scalar_select(ScalarField& f) {
  if (!f.wall_on() && !f.source_on()) return;
  std::vector<uint32_t> img(N, 0u);
  if (f.wall_on()) {
    const cfd_scalar_wall& w = f.wall;
    for (const WallFace& wfc : wall_faces)
      if (wfc.cx >= w.x0 && wfc.cx <= w.x1 && wfc.cy >= w.y0 && wfc.cy <= w.y1) img[wfc.cell] |= 1u << wfc.slot;
  }
  if (f.source_on()) {
    const cfd_scalar_source& q = f.source;
    for (uint32_t i = 0; i < N; ++i)
      if (cell_cx[i] >= q.x0 && cell_cx[i] <= q.x1 && cell_cy[i] >= q.y0 && cell_cy[i] <= q.y1) img[i] |= 1u << 31;
  }
  CFD_HIP(hipSetDevice(device));
  if (!f.sel) f.sel = sc_arena.alloc<uint32_t>(N);
  CFD_HIP(hipMemcpyAsync(f.sel, img.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  sync();
}

uint32_t Solver::set_scalar_wall(int field, const cfd_scalar_wall& c) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar wall on a distributed handle");
  scalar_check(field);
  if (c.kind < 0 || c.kind > 2)
    throw std::invalid_argument("scalar wall: kind must be 0 (adiabatic), 1 (fixed value) or 2 (fixed flux)");
  if (!std::isfinite(c.value)) throw std::invalid_argument("scalar wall: value must be finite");
  uint32_t count = 0;
  if (!(c.x1 < c.x0))
    for (const WallFace& wfc : wall_faces) {
      if (!(wfc.cx >= c.x0 && wfc.cx <= c.x1 && wfc.cy >= c.y0 && wfc.cy <= c.y1)) continue;
      if (c.kind != 0 && wfc.slot >= 31)
        throw std::invalid_argument("scalar wall keeps a cell's selected wall slots in 31 bits: wall face at slot 31 or "
                                    "above of its cell");
      ++count;
    }
  ScalarField& f = sc_field[field];
  f.wall = c;
  f.wall_n = count;
  ++surface_gen;  // a surface re-derives its channels and resets its statistics (surface.cpp)
  scalar_select(f);
  return count;
}

uint32_t Solver::set_scalar_source(int field, const cfd_scalar_source& c) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar source on a distributed handle");
  scalar_check(field);
  if (!std::isfinite(c.rate)) throw std::invalid_argument("scalar source: rate must be finite");
  uint32_t count = 0;
  if (!(c.x1 < c.x0))
    for (uint32_t i = 0; i < N; ++i)
      if (cell_cx[i] >= c.x0 && cell_cx[i] <= c.x1 && cell_cy[i] >= c.y0 && cell_cy[i] <= c.y1) ++count;
  ScalarField& f = sc_field[field];
  f.source = c;
  f.source_n = count;
  scalar_select(f);
  return count;
}

// Read-only on the current field, with the current density and diffusivity; a
// field without selected faces launches nothing.
void Solver::scalar_wall_flux(int field, cfd_scalar_wall_flux* out) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no scalar wall flux on a distributed handle");
  scalar_check(field);
  const ScalarField& f = sc_field[field];
  std::memset(out, 0, sizeof(*out));
  out->faces = f.wall_n;
  out->kind = f.wall.kind;
  if (!f.wall_on()) return;
  CFD_HIP(hipSetDevice(device));
  ScalarWallFluxArgs a{};
  a.N = N;
  a.area = fs.area;
  a.dist_e = fs.dist_e;
  a.sel = f.sel;
  a.phi = f.phi;
  a.rd = constants.density * f.par.diffusivity;
  a.kind = f.wall.kind;
  a.value = f.wall.value;
  a.out = sum_buf(wf_sums, kWallFluxSums, sc_arena);
  launch_scalar_wall_flux(a, stream);
  double h[kWallFluxSums];
  sum_read(wf_sums, kWallFluxSums, h, "scalar wall flux");
  out->flux = h[0];
  out->area = h[1];
  out->phi_area = h[2];
}

// ---- Boussinesq buoyancy ----
void Solver::set_buoyancy(int field, float beta, float ref) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no buoyancy on a distributed handle");
  scalar_check(field);
  if (!std::isfinite(beta) || !std::isfinite(ref)) throw std::invalid_argument("scalar buoyancy: beta and ref must be finite");
  sc_field[field].beta = beta;
  sc_field[field].bref = ref;
}

void Solver::set_gravity(float gx, float gy) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no gravity on a distributed handle");
  if (!std::isfinite(gx) || !std::isfinite(gy)) throw std::invalid_argument("gravity: g_x and g_y must be finite");
  gravity[0] = gx;
  gravity[1] = gy;
}

// The field pointers are read here, at launch time: f.phi swaps with sc_alt
// during an advance.
bool Solver::buoyancy_args(BuoyancyArgs& b) const {
  b = BuoyancyArgs{};
  for (int fi = 0; fi < sc_count; ++fi) {
    const ScalarField& f = sc_field[fi];
    if (f.beta != 0.0f) b.f[b.n++] = BuoyancyField{f.phi, f.beta, f.bref};
  }
  b.gx = gravity[0];
  b.gy = gravity[1];
  return b.n > 0 && (b.gx != 0.0f || b.gy != 0.0f);
}

void Solver::buoyancy_get(cfd_buoyancy* out) const {
  std::memset(out, 0, sizeof(*out));
  out->gx = gravity[0];
  out->gy = gravity[1];
  out->fields = sc_count;
  for (int fi = 0; fi < sc_count; ++fi) {
    out->beta[fi] = sc_field[fi].beta;
    out->ref[fi] = sc_field[fi].bref;
  }
  BuoyancyArgs b;
  out->active = buoyancy_args(b) ? 1 : 0;
}

// Read-only on the current fields, with the current density; launches nothing
// unless the assembly would take its buoyant form.
void Solver::buoyancy_force(cfd_buoyancy_force* out) {
  if (dist()) throw std::invalid_argument("passive scalars run on one GPU only: no buoyancy force on a distributed handle");
  if (sc_count == 0) throw std::invalid_argument("passive scalars are not enabled (cfd_scalars_enable)");
  std::memset(out, 0, sizeof(*out));
  BuoyancyForceArgs a{};
  const bool on = buoyancy_args(a.b);
  out->fields = (uint32_t)a.b.n;
  if (!on) return;
  CFD_HIP(hipSetDevice(device));
  a.N = N;
  a.vol = d_vol;
  a.density = constants.density;
  a.out = sum_buf(bf_sums, kBuoyancySums, sc_arena);
  launch_buoyancy_force(a, stream);
  double h[kBuoyancySums];
  sum_read(bf_sums, kBuoyancySums, h, "buoyancy force");
  out->force[0] = h[0];
  out->force[1] = h[1];
}

void Solver::scalar_stats(int field, cfd_scalar_stats* out) {
  scalar_check(field);
  CFD_HIP(hipSetDevice(device));
  const ScalarField& f = sc_field[field];
  ScalarStatsArgs a{};
  a.N = N;
  a.vol = d_vol;
  a.phi = f.phi;
  a.out = sum_out(sc_partial);
  a.blockmm = sc_blockmax;
  launch_scalar_stats(a, sc_res, stream);
  launch_evolution_final(combine(sc_partial, 1), &sc_res->integral, stream);
  check_launch("scalar stats");
  ScalarResults h;
  CFD_HIP(hipMemcpyAsync(&h, sc_res, sizeof(h), hipMemcpyDeviceToHost, stream));
  sync();
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
