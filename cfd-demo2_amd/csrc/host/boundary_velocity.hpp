// Prescribed boundary velocities and the wall-motion sums (boundary_velocity.cpp;
// kernels.hpp BcvArgs, WallMotionArgs): a plain struct the Solver holds one of.
// Opt-in: nothing is allocated before the first non-empty set, and with an
// empty selection step() launches the kernels it always launched.  Every
// method takes the solver as a const FlowView.  One GPU only and not in
// reference-semantics mode: Solver::bcv_need refuses both before a call.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "flow_view.hpp"
#include "topology.hpp"

namespace cfd2 {

struct BoundaryVelocity {
  struct Entry {
    float bx, by;
    uint32_t btype;
  };
  std::vector<BndFace> faces;                      // boundary_faces of the mesh (one GPU)
  std::vector<std::pair<uint32_t, Entry>> sel;     // (index into faces, entry), ascending
  DeviceArena arena;
  uint32_t* dsel = nullptr;   // [N]; null: empty selection
  float4* dtab = nullptr;     // [rows * wf]
  float scale[2] = {1.0f, 1.0f};  // inlet, wall
  double max_normal = 0.0;    // largest |v . n| removed from a wall entry of the current selection
  uint64_t gen = 0;  // set: a surface re-derives its channels and resets its statistics (FlowView::surface_gen)
  // wall-motion sums over the force region: the compact table of the region's
  // f64 face centres is rebuilt when the region changed (ForceRegion::gen)
  DeviceArena wm_arena;
  uint32_t* wm_crow = nullptr;    // [N]
  double2* wm_ctr = nullptr;      // [rows * wf]
  SumBuf wm_sums;                 // kWallMotionSums, in wm_arena
  uint64_t wm_gen = 0;            // the region wm_crow / wm_ctr were built for

  bool on() const { return dsel != nullptr; }
  BcvArgs args() const { return BcvArgs{dsel, dtab, scale[0], scale[1]}; }
  // throws what a call named `what` says on a distributed handle and in reference-semantics mode
  static void need(const char* what, bool dist, bool ref_racy);
  uint32_t set(const FlowView& flow, uint32_t n, const uint32_t* face_ids, const float* vx, const float* vy);
  void set_scale(const FlowView& flow, float inlet_scale, float wall_scale);
  void get(const FlowView& flow, cfd_boundary_velocity* out) const;
  // wall: every wall face of the mesh
  void wall_motion(const FlowView& flow, const ForceRegion& region, const std::vector<WallFace>& wall, double x0,
                   double y0, cfd_wall_motion* out);
};

}  // namespace cfd2
