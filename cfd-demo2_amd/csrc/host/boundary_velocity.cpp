// Prescribed boundary velocities (include/cfd2_amd.h "Arithmetic of boundary
// velocities"; kernels.hpp BcvArgs): the selection of inlet and wall faces with
// a velocity of their own, its compact device image, the two scale factors and
// the wall-motion sums over the force region.
#include <cmath>
#include <cstring>

#include <algorithm>

#include "boundary_velocity.hpp"

namespace cfd2 {

void BoundaryVelocity::need(const char* what, bool dist, bool ref_racy) {
  if (dist) throw std::invalid_argument(std::string("boundary velocities run on one GPU only: no ") + what + " on a distributed handle");
  if (ref_racy)
    throw std::invalid_argument(std::string("boundary velocities: no ") + what +
                                " in reference-semantics mode (the racy prepare has no such form)");
}

// Every face is checked before anything changes.  The device image is rebuilt
// as a whole: one row of wf entries per cell with a selected slot.
uint32_t BoundaryVelocity::set(const FlowView& flow, uint32_t n, const uint32_t* face_ids, const float* vx,
                               const float* vy) {
  std::vector<std::pair<uint32_t, Entry>> add;
  add.reserve(n);
  double max_removed = 0.0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t f = face_ids[j];
    auto it = std::lower_bound(faces.begin(), faces.end(), f,
                               [](const BndFace& b, uint32_t face) { return b.face < face; });
    if (it == faces.end() || it->face != f)
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
    add.push_back({(uint32_t)(it - faces.begin()), Entry{(float)x, (float)y, it->btype}});
  }
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();  // no kernel reads the old image any more
  ++gen;
  if (n == 0) {
    sel.clear();
    max_normal = 0.0;
  } else {
    // a later entry replaces an earlier one of the same face, within this call too
    std::stable_sort(add.begin(), add.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<std::pair<uint32_t, Entry>> merged;
    size_t i = 0, j = 0;
    while (i < sel.size() || j < add.size()) {
      if (j == add.size() || (i < sel.size() && sel[i].first < add[j].first)) {
        merged.push_back(sel[i++]);
        continue;
      }
      if (i < sel.size() && sel[i].first == add[j].first) ++i;
      while (j + 1 < add.size() && add[j + 1].first == add[j].first) ++j;
      merged.push_back(add[j++]);
    }
    sel.swap(merged);
    max_normal = std::fmax(max_normal, max_removed);
  }
  arena.release();
  dsel = nullptr;
  dtab = nullptr;
  if (sel.empty()) return 0;
  const uint32_t wf = (uint32_t)flow.fs.wf;
  std::vector<uint32_t> row(flow.N, 0u);
  std::vector<float4> tab;
  for (const auto& s : sel) {
    const BndFace& b = faces[s.first];
    if (b.slot >= wf) throw std::logic_error("boundary velocity: face slot beyond the slot width");
    if (row[b.cell] == 0u) {
      tab.resize(tab.size() + wf, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
      row[b.cell] = (uint32_t)(tab.size() / wf);
    }
    tab[(size_t)(row[b.cell] - 1u) * wf + b.slot] =
        make_float4(s.second.bx, s.second.by, s.second.btype == 1u ? kBcvInlet : kBcvWall, 0.0f);
  }
  uint32_t* up_sel = arena.upload(row, flow.stream);
  float4* up_tab = arena.upload(tab, flow.stream);
  flow.sync();
  dsel = up_sel;
  dtab = up_tab;
  return (uint32_t)sel.size();
}

// Kernel arguments: a change takes effect at the next launch of prepare /
// assemble, which a step never replays from a captured graph.
void BoundaryVelocity::set_scale(const FlowView&, float inlet_scale, float wall_scale) {
  if (!std::isfinite(inlet_scale) || !std::isfinite(wall_scale))
    throw std::invalid_argument("boundary velocity scale: both factors must be finite");
  scale[0] = inlet_scale;
  scale[1] = wall_scale;
}

void BoundaryVelocity::get(const FlowView&, cfd_boundary_velocity* out) const {
  std::memset(out, 0, sizeof(*out));
  for (const auto& s : sel) (s.second.btype == 1u ? out->inlet_faces : out->wall_faces)++;
  out->inlet_scale = scale[0];
  out->wall_scale = scale[1];
  out->active = on() ? 1 : 0;
  out->max_normal_removed = max_normal;
}

// Read-only on the current state; an empty force region launches nothing.
void BoundaryVelocity::wall_motion(const FlowView& flow, const ForceRegion& region, const std::vector<WallFace>& wall,
                                   double x0, double y0, cfd_wall_motion* out) {
  if (!std::isfinite(x0) || !std::isfinite(y0)) throw std::invalid_argument("wall motion: the reference point must be finite");
  std::memset(out, 0, sizeof(*out));
  out->region_faces = region.faces;
  for (const auto& s : sel) {
    const BndFace& b = faces[s.first];
    if (b.btype == 3u && region.on && region.holds(b.cx, b.cy)) out->moving_faces++;
  }
  if (!region.on) return;
  CFD_HIP(hipSetDevice(flow.device));
  const uint32_t wf = (uint32_t)flow.fs.wf;
  if (!wm_crow || wm_gen != region.gen) {
    flow.sync();
    wm_arena.release();
    wm_crow = nullptr;
    wm_sums = SumBuf{};
    std::vector<uint32_t> crow(flow.N, 0u);
    std::vector<double2> ctr;
    for (const WallFace& wfc : wall) {
      if (!region.holds(wfc.cx, wfc.cy)) continue;
      if (wfc.slot >= wf) throw std::logic_error("wall motion: face slot beyond the slot width");
      if (crow[wfc.cell] == 0u) {
        ctr.resize(ctr.size() + wf, make_double2(0.0, 0.0));
        crow[wfc.cell] = (uint32_t)(ctr.size() / wf);
      }
      ctr[(size_t)(crow[wfc.cell] - 1u) * wf + wfc.slot] = make_double2(wfc.cx, wfc.cy);
    }
    uint32_t* dcrow = wm_arena.upload(crow, flow.stream);
    wm_ctr = wm_arena.upload(ctr, flow.stream);
    flow.sync();
    wm_crow = dcrow;
    wm_gen = region.gen;
  }
  WallMotionArgs a{};
  a.N = flow.N;
  a.c = flow.constants;
  a.fs = flow.fs;
  a.u = flow.u;
  a.p = flow.p;
  a.wall_mask = region.mask;
  a.crow = wm_crow;
  a.ctr = wm_ctr;
  a.v = on() ? args() : BcvArgs{nullptr, nullptr, scale[0], scale[1]};
  a.mu = flow.visc_mu;
  a.x0 = x0;
  a.y0 = y0;
  a.out = flow.sums.buf(wm_sums, kWallMotionSums, wm_arena);
  launch_wall_motion(a, flow.stream);
  double h[kWallMotionSums];
  flow.sum_read(wm_sums, kWallMotionSums, h, "wall motion");
  out->torque_pressure = h[0];
  out->torque_viscous = h[1];
  out->power = h[2];
}

}  // namespace cfd2
