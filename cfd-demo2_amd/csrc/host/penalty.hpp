// Volume penalisation (penalty.cpp; include/cfd2_amd.h "Arithmetic of volume
// penalisation"; kernels.hpp PenaltyArgs): a drag coefficient, an optional
// Forchheimer coefficient and an optional target velocity per cell, a plain
// struct the Solver holds one of.  Opt-in: nothing is allocated before the
// first field is set, and without a field step() launches the kernels it
// always launched.  Every method takes the solver as a const FlowView.  One
// GPU only and not in reference-semantics mode: Solver::pen_need refuses both
// before a call.  A checkpoint stores none of it (as for buoyancy, the
// boundary velocities and the viscosity): a resumed run sets it again.
#pragma once
#include <cstdint>
#include <vector>

#include "flow_view.hpp"
#include "topology.hpp"

namespace cfd2 {

// min over the cells of vol, and of G_i = the sum of area / dist_a over the
// slots that enter the pressure row's diagonal (interior and outlet slots), in
// f64 from the f32 slot arrays: what the limit on vol * sigma is made of
struct PenaltyGeometry {
  double vol_min = 0.0, vol_max = 0.0, g_min = 0.0;
};
PenaltyGeometry penalty_geometry(const Topology& t);
// The largest vol[i] * sigma[i] cfd_set_penalty takes (the header derives it):
//   density * g_min * vol_min / (4 * 1e-14)
double penalty_limit(const PenaltyGeometry& g, float density);

struct Penalty {
  DeviceArena arena;
  // one allocation of 4 N floats, sigma | forch | target, made at the first
  // set and kept while a field is set: replacing the field is one upload into
  // it, and the kernels read the contents when they run
  float* buf = nullptr;
  uint32_t n = 0;
  bool has_forch = false, has_target = false;
  float scale = 1.0f;  // target_scale: a kernel argument, never uploaded
  uint64_t gen = 0;    // enabling, clearing and a change of which pointers are null: the PEN forms come and go.
                       // Nothing reads it yet (no captured graph holds prepare or the assembly); it is kept, as
                       // Viscosity::gen is, for the first consumer that caches a launch
  double2* ctr = nullptr;  // [N] f64 cell centres, uploaded at the first force()
  SumBuf sums;             // kPenaltySums, in `arena`

  bool on() const { return buf != nullptr; }
  PenaltyArgs args() const {
    return PenaltyArgs{buf, has_forch ? buf + n : nullptr,
                       has_target ? reinterpret_cast<const float2*>(buf + 2 * (size_t)n) : nullptr, scale};
  }
  // throws what a call named `what` says on a distributed handle and in
  // reference-semantics mode (ref_mode: the racy prepare or the in-place smoother is on)
  static void need(const char* what, bool dist, bool ref_mode);
  // count == N: enables or replaces the field; count == 0: clears it.  Every
  // value is checked before anything changes: finite, sigma and forch >= 0,
  // max(vol) * max(sigma) finite in f32, vol[i] * sigma[i] <= limit.
  void set(const FlowView& flow, const std::vector<float>& vol, double limit, const float* sigma, const float* forch,
           const float* target, uint32_t count);
  void set_scale(float s);
  // sigma[N], forch[N], target[2 N] (each may be null); refused without a field
  void get(const FlowView& flow, float* sigma, float* forch, float* target) const;
  // the sums of kernels.hpp PenaltyForceArgs on the current state; refused without a field
  void force(const FlowView& flow, const std::vector<double>& cx, const std::vector<double>& cy, double x0, double y0,
             const double* box, cfd_penalty_force* out);
};

}  // namespace cfd2
