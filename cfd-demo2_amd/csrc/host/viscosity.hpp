// Variable viscosity (viscosity.cpp; include/cfd2_amd.h "Arithmetic of variable
// viscosity"; kernels.hpp launch_prepare_visc): a viscosity per cell, a plain
// struct the Solver holds one of.  Opt-in: nothing is allocated before the
// first field is set, and without a field step() launches the kernels it
// always launched.  Every method takes the solver as a const FlowView.  One
// GPU only and not in reference-semantics mode: Solver::visc_need refuses both
// before a call.  A checkpoint stores neither the field nor that one is set
// (as for buoyancy and the boundary velocities): a resumed run sets it again.
#pragma once
#include <cstdint>

#include "flow_view.hpp"

namespace cfd2 {

struct Viscosity {
  DeviceArena arena;
  float* mu = nullptr;  // [N]; null: no field.  The pointer stays while a field is set: replacing the
                        // field is one upload into it, and the kernels read the contents when they run
  uint64_t gen = 0;     // enabling and clearing: the VISC forms come and go.  Not part of the view's surface_gen:
                        // a surface's channel layout does not depend on the viscosity, and its statistics stay

  bool on() const { return mu != nullptr; }
  // throws what a call named `what` says on a distributed handle and in
  // reference-semantics mode (ref_mode: the racy prepare or the in-place smoother is on)
  static void need(const char* what, bool dist, bool ref_mode);
  // n == N: enables or replaces the field; n == 0: clears it.  Every value is
  // checked (finite and > 0) before anything changes.
  void set(const FlowView& flow, const float* values, uint32_t n);
  void get(const FlowView& flow, float* out) const;  // refused without a field
  // ---- the models (kernels.hpp ViscosityModelArgs): evaluated into mu ----
  cfd_viscosity_model model{};  // kind 0: none
  float* gdot = nullptr;        // [N] the shear rate of the last evaluation, in `arena`
  uint32_t* stats = nullptr;    // [4]
  bool has_model() const { return model.kind != 0; }
  void set_model(const FlowView& flow, const cfd_viscosity_model& m);  // every parameter checked before anything changes
  void evaluate(const FlowView& flow);  // one launch on flow.stream, no synchronisation; refused without a model
  void shear_rate(const FlowView& flow, float* out) const;
  void stats_get(const FlowView& flow, cfd_viscosity_stats* out) const;
};

}  // namespace cfd2
