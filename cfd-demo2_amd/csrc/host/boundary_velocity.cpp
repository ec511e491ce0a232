// Prescribed boundary velocities (include/cfd2_amd.h "Arithmetic of boundary
// velocities"; kernels.hpp BcvArgs): the selection of inlet and wall faces with
// a velocity of their own, its compact device image, the two scale factors and
// the wall-motion sums over the force region.
#include <cmath>
#include <cstring>

#include "solver_impl.hpp"

namespace cfd2 {

void Solver::bcv_need(const char* what) const {
  if (dist()) throw std::invalid_argument(std::string("boundary velocities run on one GPU only: no ") + what + " on a distributed handle");
  if (ref_racy)
    throw std::invalid_argument(std::string("boundary velocities: no ") + what +
                                " in reference-semantics mode (the racy prepare has no such form)");
}

// Every face is checked before anything changes.  The device image is rebuilt
// as a whole: one row of wf entries per cell with a selected slot.
uint32_t Solver::set_boundary_velocity(uint32_t n, const uint32_t* faces, const float* vx, const float* vy) {
  bcv_need("boundary velocity");
  std::vector<std::pair<uint32_t, BcvEntry>> add;
  add.reserve(n);
  double max_removed = 0.0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t f = faces[j];
    auto it = std::lower_bound(bnd_faces.begin(), bnd_faces.end(), f,
                               [](const BndFace& b, uint32_t face) { return b.face < face; });
    if (it == bnd_faces.end() || it->face != f)
      throw std::invalid_argument("boundary velocity: face " + std::to_string(f) + " is not an inlet or wall boundary face");
    if (!std::isfinite(vx[j]) || !std::isfinite(vy[j])) throw std::invalid_argument("boundary velocity: velocities must be finite");
    double x = (double)vx[j], y = (double)vy[j];
    if (it->btype == 3u) {  // walls stay impermeable: the normal component goes, in f64
      const double nn = it->nx * it->nx + it->ny * it->ny;
      if (nn > 0.0) {
        const double vn = (x * it->nx + y * it->ny) / nn;
        x -= vn * it->nx;
        y -= vn * it->ny;
        max_removed = std::fmax(max_removed, std::fabs(vn) * std::sqrt(nn));
      }
    }
    add.push_back({(uint32_t)(it - bnd_faces.begin()), BcvEntry{(float)x, (float)y, it->btype}});
  }
  CFD_HIP(hipSetDevice(device));
  sync();  // no kernel reads the old image any more
  ++surface_gen;  // a surface re-derives its channels and resets its statistics (surface.cpp)
  if (n == 0) {
    bcv_sel.clear();
    bcv_max_normal = 0.0;
  } else {
    // a later entry replaces an earlier one of the same face, within this call too
    std::stable_sort(add.begin(), add.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<std::pair<uint32_t, BcvEntry>> merged;
    size_t i = 0, j = 0;
    while (i < bcv_sel.size() || j < add.size()) {
      if (j == add.size() || (i < bcv_sel.size() && bcv_sel[i].first < add[j].first)) {
        merged.push_back(bcv_sel[i++]);
        continue;
      }
      if (i < bcv_sel.size() && bcv_sel[i].first == add[j].first) ++i;
      while (j + 1 < add.size() && add[j + 1].first == add[j].first) ++j;
      merged.push_back(add[j++]);
    }
    bcv_sel.swap(merged);
    bcv_max_normal = std::fmax(bcv_max_normal, max_removed);
  }
  bcv_arena.release();
  bcv_dsel = nullptr;
  bcv_dtab = nullptr;
  if (bcv_sel.empty()) return 0;
  const uint32_t wf = (uint32_t)topo.wf;
  std::vector<uint32_t> sel(N, 0u);
  std::vector<float4> tab;
  for (const auto& s : bcv_sel) {
    const BndFace& b = bnd_faces[s.first];
    if (b.slot >= wf) throw std::logic_error("boundary velocity: face slot beyond the slot width");
    if (sel[b.cell] == 0u) {
      tab.resize(tab.size() + wf, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
      sel[b.cell] = (uint32_t)(tab.size() / wf);
    }
    tab[(size_t)(sel[b.cell] - 1u) * wf + b.slot] =
        make_float4(s.second.bx, s.second.by, s.second.btype == 1u ? kBcvInlet : kBcvWall, 0.0f);
  }
  uint32_t* dsel = bcv_arena.upload(sel, stream);
  float4* dtab = bcv_arena.upload(tab, stream);
  sync();
  bcv_dsel = dsel;
  bcv_dtab = dtab;
  return (uint32_t)bcv_sel.size();
}

// Kernel arguments: a change takes effect at the next launch of prepare /
// assemble, which a step never replays from a captured graph.
void Solver::set_boundary_velocity_scale(float inlet_scale, float wall_scale) {
  bcv_need("boundary velocity scale");
  if (!std::isfinite(inlet_scale) || !std::isfinite(wall_scale))
    throw std::invalid_argument("boundary velocity scale: both factors must be finite");
  bcv_scale[0] = inlet_scale;
  bcv_scale[1] = wall_scale;
}

void Solver::boundary_velocity_get(cfd_boundary_velocity* out) const {
  std::memset(out, 0, sizeof(*out));
  for (const auto& s : bcv_sel) (s.second.btype == 1u ? out->inlet_faces : out->wall_faces)++;
  out->inlet_scale = bcv_scale[0];
  out->wall_scale = bcv_scale[1];
  out->active = bcv_on() ? 1 : 0;
  out->max_normal_removed = bcv_max_normal;
}

// Read-only on the current state; an empty force region launches nothing.
void Solver::wall_motion(double x0, double y0, cfd_wall_motion* out) {
  bcv_need("wall motion");
  if (!std::isfinite(x0) || !std::isfinite(y0)) throw std::invalid_argument("wall motion: the reference point must be finite");
  std::memset(out, 0, sizeof(*out));
  out->region_faces = region_faces;
  for (const auto& s : bcv_sel) {
    const BndFace& b = bnd_faces[s.first];
    if (b.btype == 3u && region_on && b.cx >= region_box[0] && b.cx <= region_box[2] && b.cy >= region_box[1] &&
        b.cy <= region_box[3])
      out->moving_faces++;
  }
  if (!region_on) return;
  CFD_HIP(hipSetDevice(device));
  const uint32_t wf = (uint32_t)topo.wf;
  if (!wm_crow || wm_gen != region_gen) {
    sync();
    wm_arena.release();
    wm_crow = nullptr;
    wm_sums = SumBuf{};
    std::vector<uint32_t> crow(N, 0u);
    std::vector<double2> ctr;
    for (const WallFace& wfc : wall_faces) {
      if (!(wfc.cx >= region_box[0] && wfc.cx <= region_box[2] && wfc.cy >= region_box[1] && wfc.cy <= region_box[3]))
        continue;
      if (wfc.slot >= wf) throw std::logic_error("wall motion: face slot beyond the slot width");
      if (crow[wfc.cell] == 0u) {
        ctr.resize(ctr.size() + wf, make_double2(0.0, 0.0));
        crow[wfc.cell] = (uint32_t)(ctr.size() / wf);
      }
      ctr[(size_t)(crow[wfc.cell] - 1u) * wf + wfc.slot] = make_double2(wfc.cx, wfc.cy);
    }
    uint32_t* dcrow = wm_arena.upload(crow, stream);
    wm_ctr = wm_arena.upload(ctr, stream);
    sync();
    wm_crow = dcrow;
    wm_gen = region_gen;
  }
  WallMotionArgs a{};
  a.N = N;
  a.c = constants;
  a.fs = fs;
  a.u = S().u;
  a.p = S().p;
  a.wall_mask = diag_mask;
  a.crow = wm_crow;
  a.ctr = wm_ctr;
  a.v = bcv_on() ? bcv_args() : BcvArgs{nullptr, nullptr, bcv_scale[0], bcv_scale[1]};
  a.x0 = x0;
  a.y0 = y0;
  a.out = sum_buf(wm_sums, kWallMotionSums, wm_arena);
  launch_wall_motion(a, stream);
  double h[kWallMotionSums];
  sum_read(wm_sums, kWallMotionSums, h, "wall motion");
  out->torque_pressure = h[0];
  out->torque_viscous = h[1];
  out->power = h[2];
}

}  // namespace cfd2
