// Passive scalars and Boussinesq buoyancy (scalar.cpp; kernels.hpp
// "scalar.hip"): a plain struct the Solver holds one of.  Opt-in: nothing is
// allocated before enable, and step() launches none of it; the assembly only
// asks buoyancy_args for its source.  Every method takes the solver as a const
// FlowView and writes only buffers of its own arena: the fields, the assembled
// system and the work space.  One GPU only; the calls that refuse a
// distributed handle do so in words of their own, so they take
// Solver::view(nullptr).
#pragma once
#include <cstdint>
#include <vector>

#include "flow_view.hpp"
#include "topology.hpp"

namespace cfd2 {

struct ScalarField {
  float* phi = nullptr;  // [ld] the current iterate (swaps with Scalars::State::alt during an advance)
  cfd_scalar_params par{};
  uint32_t sweeps = 0;
  int32_t converged = 0;
  float last_delta = 0.0f;
  float dt_used = 0.0f;
  cfd_scalar_solver solver{0, 500, 8, 0};  // cfd_scalar_solver_default
  cfd_scalar_solver_stats kstats{};        // of the last advance
  int32_t scheme = 0;                      // cfd_scalar_scheme.scheme, for the next advance
  int32_t scheme_used = 0;                 // of the last advance
  uint32_t clamped = 0;                    // of the last advance (copied from hr_count during it)
  // wall condition and source (cfd_set_scalar_wall / cfd_set_scalar_source), for the next advance
  cfd_scalar_wall wall{};                  // kind 0: every wall adiabatic
  cfd_scalar_source source{};              // rate 0: none
  uint32_t wall_n = 0;                     // wall faces in wall's box
  uint32_t source_n = 0;                   // cells in source's box
  uint32_t* sel = nullptr;                 // [N] the selection image (kernels.hpp ScalarBC), null before the first non-trivial selection
  // Boussinesq buoyancy (set_buoyancy): the field drives the momentum equation when beta != 0
  float beta = 0.0f;
  float bref = 0.0f;
  bool wall_on() const { return wall.kind != 0 && wall_n != 0; }
  bool source_on() const { return source.rate != 0.0f && source_n != 0; }
};

struct Scalars {
  DeviceArena arena;  // every buffer below; released by enable
  // what enable resets as a whole (every beta with it: the step is the plain one again)
  struct State {
    int count = 0;
    ScalarField field[4];
    float* alt = nullptr;         // [ld] ping-pong partner of the field being advanced
    float* coef = nullptr;        // [wf * ld] slot coefficients of the field being advanced
    float* diag = nullptr;        // [ld]
    float* b = nullptr;           // [ld]
    uint32_t* blockmax = nullptr; // per-block scratch of the sweep's delta and the stats' min / max
    ScalarResults* res = nullptr; // what the sweep and the statistics leave for the host
    double* partial = nullptr;    // [pstride] unit partials of the integral
    // BiCGStab work space, allocated by the first set_solver that selects method 1 (null before)
    float* kr_vec[6] = {};        // [ld] each: rh, r, p, v, s, t
    double* kr_partial = nullptr; // [2 * pstride] unit partials of an iteration's dots
    ScalarKrylovState* kr_state = nullptr;
    // Scheme 1 (limited linear) work space, allocated by the first set_scheme that selects it (null before)
    float2* hr_grad = nullptr;    // [ld] the gradient of the phi_old being advanced
    uint32_t* hr_count = nullptr; // [4] clamped cells of each field's last scheme-1 assembly
    // Wall-flux and buoyancy-force work space, allocated by the first wall_flux
    // that has faces to sum over and the first buoyancy_force with buoyancy on
    SumBuf wf_sums;               // kWallFluxSums: flux, area, phi_area
    SumBuf bf_sums;               // kBuoyancySums
  } s;
  cfd_scalar_config cfg{};
  float gravity[2] = {0.0f, 0.0f};  // set_gravity; kept over enable
  uint64_t gen = 0;  // enable and set_wall: a surface re-derives its channels and resets its statistics (FlowView::surface_gen)

  void enable(const FlowView& flow, int count, const cfd_scalar_config& c);
  void check(int field) const { scalar_index_check(s.count, field); }  // throws: not enabled / bad index
  void set_params(const FlowView& flow, int field, const cfd_scalar_params& p);
  void set(const FlowView& flow, int field, const double* phi);
  void get(const FlowView& flow, int field, double* phi);
  void advance(const FlowView& flow, float dt);
  void set_solver(const FlowView& flow, int field, const cfd_scalar_solver& c);
  void solver_stats(const FlowView& flow, int field, cfd_scalar_solver_stats* out) const;
  void set_scheme(const FlowView& flow, int field, const cfd_scalar_scheme& c);
  void scheme_stats(const FlowView& flow, int field, cfd_scalar_scheme_stats* out) const;
  void stats(const FlowView& flow, int field, cfd_scalar_stats* out);
  // wall: every wall face of the mesh; cx, cy: the f64 cell centres.  Both return what their box selected.
  uint32_t set_wall(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
                    const std::vector<double>& cy, int field, const cfd_scalar_wall& c);
  uint32_t set_source(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
                      const std::vector<double>& cy, int field, const cfd_scalar_source& c);
  void wall_flux(const FlowView& flow, int field, cfd_scalar_wall_flux* out);
  // Boussinesq buoyancy (include/cfd2_amd.h "Arithmetic of buoyancy"): explicit,
  // one momentum source in the assembly, read from the fields as they stand
  void set_buoyancy(const FlowView& flow, int field, float beta, float ref);
  void set_gravity(const FlowView& flow, float gx, float gy);
  // the driving fields (beta != 0, ascending) with their current pointers and
  // g; true when the assembly takes its buoyant form (some entry and g != 0)
  bool buoyancy_args(BuoyancyArgs& b) const;
  void buoyancy_get(const FlowView& flow, cfd_buoyancy* out) const;
  void buoyancy_force(const FlowView& flow, cfd_buoyancy_force* out);
  // what the post-processing modules read of field f (FlowView::field); zeros beyond count
  SurfaceField surface_field(int f, float density) const;

 private:
  ScalarSystem system(const FlowView& flow) const;  // the assembled system of the field being advanced
  void krylov(const FlowView& flow, ScalarField& f);  // the Krylov phase of one assembled field: f.phi becomes its frozen x
  void polish(const FlowView& flow, int fi, ScalarField& f);  // the Jacobi loop from f.phi: sweeps, last_delta, converged
  // f.sel from f.wall and f.source (allocates and uploads it when either is on)
  void select(const FlowView& flow, const std::vector<WallFace>& wall, const std::vector<double>& cx,
              const std::vector<double>& cy, ScalarField& f);
};

}  // namespace cfd2
