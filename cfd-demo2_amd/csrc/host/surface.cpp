// Wall surface distributions (include/cfd2_amd.h "Wall surface distributions";
// kernels.hpp "surface.hip"): the face table of a box of wall faces, the
// per-face channels of the current state and their running mean and variance.
// Read-only on the solver's state; every buffer lives in the module's own arenas.
#include <cmath>
#include <cstring>

#include "solver_impl.hpp"

namespace cfd2 {

namespace {
const char* kSurfaceOneGpu = "surface distributions run on one GPU only: a distributed handle holds a part of the fields";
}  // namespace

void Solver::surface_clear() {
  CFD_HIP(hipSetDevice(device));
  sync();
  sf_arena.release();
  sf_ch_arena.release();
  sf_on = false;
  sf_face.clear();
  sf_cell = sf_slot = nullptr;
  sf_ld = 0;
  sf_nch = 0;
  sf_out = sf_mean = sf_m2 = nullptr;
  sf_stats = false;
  sf_W = 0.0;
  sf_samples = 0;
}

// The channel buffers for the scalar fields enabled now.  The statistics keep
// their on / off state and start afresh: a mean over samples of two different
// channel sets, wall selections or wall conditions means nothing.
void Solver::surface_derive() {
  CFD_HIP(hipSetDevice(device));
  sync();
  sf_ch_arena.release();
  sf_mean = sf_m2 = nullptr;
  sf_nch = surface_channels((uint32_t)sc_count);
  const size_t len = (size_t)sf_nch * sf_ld;
  sf_out = sf_ch_arena.alloc<double>(len);
  if (sf_stats) {
    sf_mean = sf_ch_arena.alloc<double>(len);
    sf_m2 = sf_ch_arena.alloc<double>(len);
    CFD_HIP(hipMemsetAsync(sf_mean, 0, len * sizeof(double), stream));
    CFD_HIP(hipMemsetAsync(sf_m2, 0, len * sizeof(double), stream));
  }
  sf_W = 0.0;
  sf_samples = 0;
  sf_gen = surface_gen;
}

void Solver::surface_need(const char* what) {
  if (dist()) throw std::invalid_argument(kSurfaceOneGpu);
  if (!sf_on) throw std::invalid_argument(std::string(what) + ": no surface is selected (cfd_surface_select)");
  if (sf_gen != surface_gen) surface_derive();
}

uint32_t Solver::surface_select(double x0, double y0, double x1, double y1) {
  if (dist()) throw std::invalid_argument(kSurfaceOneGpu);
  if (x1 < x0) {
    surface_clear();
    return 0;
  }
  std::vector<uint32_t> face = wall_faces_in_box(x0, y0, x1, y1);
  const uint32_t wf = (uint32_t)topo.wf;
  std::vector<uint32_t> cell(face.size()), slot(face.size());
  for (size_t j = 0; j < face.size(); ++j) {  // checked before anything changes: the kernels index with these
    const WallFace& w = wall_faces[face[j]];
    if (w.cell >= N || w.slot >= wf) throw std::logic_error("surface: wall face outside the face-slot arrays");
    cell[j] = w.cell;
    slot[j] = w.slot;
  }
  const bool stats = sf_on && sf_stats;  // a new surface keeps the statistics on, and resets them
  surface_clear();
  sf_cell = sf_arena.upload(cell, stream);
  sf_slot = sf_arena.upload(slot, stream);
  sync();  // the uploads read host vectors that end here
  sf_face.swap(face);
  sf_ld = std::max<size_t>(64, (sf_face.size() + 63) / 64 * 64);
  sf_stats = stats;
  sf_on = true;
  surface_derive();
  return (uint32_t)sf_face.size();
}

void Solver::surface_geometry(uint32_t* cell, uint32_t* slot, double* cx, double* cy, double* nx, double* ny, double* area,
                              double* dist_e) {
  surface_need("cfd_surface_geometry_get");
  for (size_t j = 0; j < sf_face.size(); ++j) {
    const WallFace& w = wall_faces[sf_face[j]];
    const size_t e = (size_t)w.slot * N + w.cell;  // the f32 values the kernels read
    if (cell) cell[j] = w.cell;
    if (slot) slot[j] = w.slot;
    if (cx) cx[j] = w.cx;
    if (cy) cy[j] = w.cy;
    if (nx) nx[j] = (double)topo.fs_nx[e];
    if (ny) ny[j] = (double)topo.fs_ny[e];
    if (area) area[j] = (double)topo.fs_area[e];
    if (dist_e) dist_e[j] = (double)topo.fs_dist_e[e];
  }
}

void Solver::surface_info(cfd_surface_info* out) {
  surface_need("cfd_surface_info_get");
  std::memset(out, 0, sizeof(*out));
  out->faces = (uint32_t)sf_face.size();
  out->channels = sf_nch;
  out->samples = sf_samples;
  out->total_weight = sf_W;
  out->stats_on = sf_stats ? 1 : 0;
}

SurfaceArgs Solver::surface_args() {
  SurfaceArgs a{};
  a.n = (uint32_t)sf_face.size();
  a.N = N;
  a.nf = (uint32_t)sc_count;
  a.cell = sf_cell;
  a.slot = sf_slot;
  a.c = constants;
  a.u = S().u;
  a.p = S().p;
  a.area = fs.area;
  a.nx = fs.nx;
  a.ny = fs.ny;
  a.dist_e = fs.dist_e;
  a.wf = (uint32_t)fs.wf;
  for (int f = 0; f < sc_count; ++f) {
    const ScalarField& s = sc_field[f];
    SurfaceField& d = a.f[f];
    d.phi = s.phi;
    d.sel = s.wall_on() ? s.sel : nullptr;  // scalar_wall_flux's own condition
    d.rd = constants.density * s.par.diffusivity;
    d.kind = s.wall.kind;
    d.value = s.wall.value;
  }
  a.ld = sf_ld;
  a.out = sf_out;
  a.mean = sf_mean;
  a.m2 = sf_m2;
  return a;
}

void Solver::surface_sample(double* out) {
  surface_need("cfd_surface_sample");
  const size_t n = sf_face.size();
  if (n == 0) return;
  const Range range("surface sample");
  CFD_HIP(hipSetDevice(device));
  const SurfaceArgs a = surface_args();
  const BcvArgs bcv = bcv_args();
  launch_surface_sample(a, bcv_on() ? &bcv : nullptr, stream);
  check_launch("surface sample");
  CFD_HIP(hipMemcpy2DAsync(out, n * sizeof(double), sf_out, sf_ld * sizeof(double), n * sizeof(double), sf_nch,
                           hipMemcpyDeviceToHost, stream));
  sync();
}

void Solver::surface_stats_enable(bool on) {
  surface_need("cfd_surface_stats_enable");
  if (on == sf_stats) return;
  sf_stats = on;
  surface_derive();
}

void Solver::surface_stats_reset() {
  surface_need("cfd_surface_stats_reset");
  if (!sf_stats) throw std::invalid_argument("cfd_surface_stats_reset: surface statistics are not enabled (cfd_surface_stats_enable)");
  CFD_HIP(hipSetDevice(device));
  const size_t len = (size_t)sf_nch * sf_ld;
  CFD_HIP(hipMemsetAsync(sf_mean, 0, len * sizeof(double), stream));
  CFD_HIP(hipMemsetAsync(sf_m2, 0, len * sizeof(double), stream));
  sf_W = 0.0;
  sf_samples = 0;
}

void Solver::surface_stats_accumulate(double weight) {
  surface_need("cfd_surface_stats_accumulate");
  if (!sf_stats)
    throw std::invalid_argument("cfd_surface_stats_accumulate: surface statistics are not enabled (cfd_surface_stats_enable)");
  if (!std::isfinite(weight)) throw std::invalid_argument("cfd_surface_stats_accumulate: the weight must be finite");
  if (!(weight > 0.0)) {
    if (!(last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_surface_stats_accumulate: weight <= 0 asks for the dt of the last cfd_step, and there was none");
    weight = (double)last_step_dt;
  }
  const Range range("surface statistics");
  CFD_HIP(hipSetDevice(device));
  const double Wn = sf_W + weight;
  SurfaceArgs a = surface_args();
  a.w = weight;
  a.r = weight / Wn;
  const BcvArgs bcv = bcv_args();
  launch_surface_accumulate(a, bcv_on() ? &bcv : nullptr, stream);
  check_launch("surface statistics");
  sf_W = Wn;
  sf_samples += 1;
}

void Solver::surface_stats_get(int kind, double* out) {
  surface_need("cfd_surface_stats_get");
  if (!sf_stats) throw std::invalid_argument("cfd_surface_stats_get: surface statistics are not enabled (cfd_surface_stats_enable)");
  if (kind != 0 && kind != 1) throw std::invalid_argument("cfd_surface_stats_get: kind must be 0 (mean) or 1 (variance)");
  const size_t n = sf_face.size();
  if (n == 0) return;
  CFD_HIP(hipSetDevice(device));
  CFD_HIP(hipMemcpy2DAsync(out, n * sizeof(double), kind == 0 ? sf_mean : sf_m2, sf_ld * sizeof(double), n * sizeof(double),
                           sf_nch, hipMemcpyDeviceToHost, stream));
  sync();
  if (kind == 1 && sf_W > 0.0)  // W == 0: every M2 is +0 and stays
    for (size_t q = 0; q < (size_t)sf_nch * n; ++q) out[q] = out[q] / sf_W;
}

}  // namespace cfd2
