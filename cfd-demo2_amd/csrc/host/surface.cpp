// Wall surface distributions (include/cfd2_amd.h "Wall surface distributions";
// kernels.hpp "surface.hip"): the face table of a box of wall faces, the
// per-face channels of the current state and their running mean and variance.
// Read-only on the solver's state by its type: the solver arrives as a const
// FlowView, pointers to const, and this file does not see the Solver.  Every
// buffer lives in the module's own arenas.
#include <cmath>
#include <cstring>

#include "modules.hpp"

namespace cfd2 {

void SurfaceDist::clear(const FlowView& flow) {
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();
  arena.release();
  ch_arena.release();
  on = false;
  face.clear();
  cell = slot = nullptr;
  ld = 0;
  nch = 0;
  out = mean = m2 = nullptr;
  stats = false;
  W = 0.0;
  samples = 0;
}

// The channel buffers for the scalar fields enabled now.  The statistics keep
// their on / off state and start afresh: a mean over samples of two different
// channel sets, wall selections or wall conditions means nothing.
void SurfaceDist::derive(const FlowView& flow) {
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();
  ch_arena.release();
  mean = m2 = nullptr;
  nch = surface_channels((uint32_t)flow.nf);
  const size_t len = (size_t)nch * ld;
  out = ch_arena.alloc<double>(len);
  if (stats) {
    mean = ch_arena.alloc<double>(len);
    m2 = ch_arena.alloc<double>(len);
    CFD_HIP(hipMemsetAsync(mean, 0, len * sizeof(double), flow.stream));
    CFD_HIP(hipMemsetAsync(m2, 0, len * sizeof(double), flow.stream));
  }
  W = 0.0;
  samples = 0;
  gen = flow.surface_gen;
}

void SurfaceDist::need(const FlowView& flow, const char* what) {
  if (!on) throw std::invalid_argument(std::string(what) + ": no surface is selected (cfd_surface_select)");
  if (gen != flow.surface_gen) derive(flow);
}

uint32_t SurfaceDist::select(const FlowView& flow, const std::vector<WallFace>& wall, double x0, double y0, double x1,
                             double y1) {
  if (x1 < x0) {
    clear(flow);
    return 0;
  }
  std::vector<uint32_t> sel = wall_faces_in_box(wall, x0, y0, x1, y1);
  const uint32_t wf = (uint32_t)flow.fs.wf;
  std::vector<uint32_t> hcell(sel.size()), hslot(sel.size());
  for (size_t j = 0; j < sel.size(); ++j) {  // checked before anything changes: the kernels index with these
    const WallFace& w = wall[sel[j]];
    if (w.cell >= flow.N || w.slot >= wf) throw std::logic_error("surface: wall face outside the face-slot arrays");
    hcell[j] = w.cell;
    hslot[j] = w.slot;
  }
  const bool keep_stats = on && stats;  // a new surface keeps the statistics on, and resets them
  clear(flow);
  cell = arena.upload(hcell, flow.stream);
  slot = arena.upload(hslot, flow.stream);
  flow.sync();  // the uploads read host vectors that end here
  face.swap(sel);
  ld = std::max<size_t>(64, (face.size() + 63) / 64 * 64);
  stats = keep_stats;
  on = true;
  derive(flow);
  return (uint32_t)face.size();
}

void SurfaceDist::geometry(const FlowView& flow, const std::vector<WallFace>& wall, const Topology& topo,
                           uint32_t* cell_out, uint32_t* slot_out, double* cx, double* cy, double* nx, double* ny,
                           double* area, double* dist_e) {
  need(flow, "cfd_surface_geometry_get");
  for (size_t j = 0; j < face.size(); ++j) {
    const WallFace& w = wall[face[j]];
    const size_t e = (size_t)w.slot * flow.N + w.cell;  // the f32 values the kernels read
    if (cell_out) cell_out[j] = w.cell;
    if (slot_out) slot_out[j] = w.slot;
    if (cx) cx[j] = w.cx;
    if (cy) cy[j] = w.cy;
    if (nx) nx[j] = (double)topo.fs_nx[e];
    if (ny) ny[j] = (double)topo.fs_ny[e];
    if (area) area[j] = (double)topo.fs_area[e];
    if (dist_e) dist_e[j] = (double)topo.fs_dist_e[e];
  }
}

void SurfaceDist::info(const FlowView& flow, cfd_surface_info* info_out) {
  need(flow, "cfd_surface_info_get");
  std::memset(info_out, 0, sizeof(*info_out));
  info_out->faces = (uint32_t)face.size();
  info_out->channels = nch;
  info_out->samples = samples;
  info_out->total_weight = W;
  info_out->stats_on = stats ? 1 : 0;
}

SurfaceArgs SurfaceDist::args(const FlowView& flow) const {
  SurfaceArgs a{};
  a.n = (uint32_t)face.size();
  a.N = flow.N;
  a.nf = (uint32_t)flow.nf;
  a.cell = cell;
  a.slot = slot;
  a.c = flow.constants;
  a.u = flow.u;
  a.p = flow.p;
  a.area = flow.fs.area;
  a.nx = flow.fs.nx;
  a.ny = flow.fs.ny;
  a.dist_e = flow.fs.dist_e;
  a.wf = (uint32_t)flow.fs.wf;
  for (int f = 0; f < flow.nf; ++f) a.f[f] = flow.field[f];
  a.ld = ld;
  a.out = out;
  a.mean = mean;
  a.m2 = m2;
  return a;
}

void SurfaceDist::sample(const FlowView& flow, double* sample_out) {
  need(flow, "cfd_surface_sample");
  const size_t n = face.size();
  if (n == 0) return;
  const Range range("surface sample");
  CFD_HIP(hipSetDevice(flow.device));
  const SurfaceArgs a = args(flow);
  launch_surface_sample(a, flow.bcv(), flow.visc_mu, flow.stream);
  flow.check_launch("surface sample");
  CFD_HIP(hipMemcpy2DAsync(sample_out, n * sizeof(double), out, ld * sizeof(double), n * sizeof(double), nch,
                           hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

void SurfaceDist::stats_enable(const FlowView& flow, bool enable) {
  need(flow, "cfd_surface_stats_enable");
  if (enable == stats) return;
  stats = enable;
  derive(flow);
}

void SurfaceDist::stats_reset(const FlowView& flow) {
  need(flow, "cfd_surface_stats_reset");
  if (!stats) throw std::invalid_argument("cfd_surface_stats_reset: surface statistics are not enabled (cfd_surface_stats_enable)");
  CFD_HIP(hipSetDevice(flow.device));
  const size_t len = (size_t)nch * ld;
  CFD_HIP(hipMemsetAsync(mean, 0, len * sizeof(double), flow.stream));
  CFD_HIP(hipMemsetAsync(m2, 0, len * sizeof(double), flow.stream));
  W = 0.0;
  samples = 0;
}

void SurfaceDist::stats_accumulate(const FlowView& flow, double weight) {
  need(flow, "cfd_surface_stats_accumulate");
  if (!stats)
    throw std::invalid_argument("cfd_surface_stats_accumulate: surface statistics are not enabled (cfd_surface_stats_enable)");
  if (!std::isfinite(weight)) throw std::invalid_argument("cfd_surface_stats_accumulate: the weight must be finite");
  if (!(weight > 0.0)) {
    if (!(flow.last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_surface_stats_accumulate: weight <= 0 asks for the dt of the last cfd_step, and there was none");
    weight = (double)flow.last_step_dt;
  }
  const Range range("surface statistics");
  CFD_HIP(hipSetDevice(flow.device));
  const double Wn = W + weight;
  SurfaceArgs a = args(flow);
  a.w = weight;
  a.r = weight / Wn;
  launch_surface_accumulate(a, flow.bcv(), flow.visc_mu, flow.stream);
  flow.check_launch("surface statistics");
  W = Wn;
  samples += 1;
}

void SurfaceDist::stats_get(const FlowView& flow, int kind, double* stats_out) {
  need(flow, "cfd_surface_stats_get");
  if (!stats) throw std::invalid_argument("cfd_surface_stats_get: surface statistics are not enabled (cfd_surface_stats_enable)");
  if (kind != 0 && kind != 1) throw std::invalid_argument("cfd_surface_stats_get: kind must be 0 (mean) or 1 (variance)");
  const size_t n = face.size();
  if (n == 0) return;
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemcpy2DAsync(stats_out, n * sizeof(double), kind == 0 ? mean : m2, ld * sizeof(double), n * sizeof(double),
                           nch, hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  if (kind == 1 && W > 0.0)  // W == 0: every M2 is +0 and stays
    for (size_t q = 0; q < (size_t)nch * n; ++q) stats_out[q] = stats_out[q] / W;
}

}  // namespace cfd2
