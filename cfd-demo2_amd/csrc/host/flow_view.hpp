// What an opt-in post-processing module (modules.hpp) may read of the solver:
// one value, built fresh by Solver::view for every call (the ring rotates), of
// const members and pointers to const.  A module method takes it first and
// has no other way to the solver's state.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../hip/kernels.hpp"
#include "device_mem.hpp"

namespace cfd2 {

// Launch-error check: hipGetLastError after each phase of the step (a host
// call, no synchronisation); with check_sync (cfg.log_level >= 3) the stream
// is also synchronised there, so an asynchronous kernel fault is reported at
// the phase that caused it (debug runs).
inline void check_launch(hipStream_t stream, bool check_sync, const char* where) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw HipError(std::string("kernel launch in ") + where + ": " + hipGetErrorString(e));
  if (check_sync) {
    const hipError_t e2 = hipStreamSynchronize(stream);
    if (e2 != hipSuccess) throw HipError(std::string("kernel execution in ") + where + ": " + hipGetErrorString(e2));
  }
}

// throws std::invalid_argument: no scalar field enabled / bad index
inline void scalar_index_check(int count, int field) {
  if (count == 0) throw std::invalid_argument("passive scalars are not enabled (cfd_scalars_enable)");
  if (field < 0 || field >= count)
    throw std::invalid_argument("scalar field index " + std::to_string(field) + " outside [0, " + std::to_string(count) + ")");
}

static_assert(kTimeStatsMaxFields == 4, "FlowView::field is written out for four scalar fields");

struct FlowView {
  const int device;
  const hipStream_t stream;
  const uint32_t N, NG;           // cells of this handle (one GPU: all of them) and of the whole mesh
  const FaceSlots fs;
  const cfd_constants constants;
  const float2* const u;          // [N] the current ring slot
  const float* const p;
  const int nf;                   // scalar fields enabled
  // per field: phi, and what the surface reads of its wall condition (sel null
  // unless the wall is on, rd = density * diffusivity in f32); zeros beyond nf
  const SurfaceField field[kTimeStatsMaxFields];
  const float last_step_dt;       // 0: no step yet
  const BcvArgs bcv_args;         // prescribed boundary velocities; through bcv()
  const bool bcv_on;
  const uint64_t surface_gen;     // bumped by every change of the scalar or boundary-velocity configuration
  const bool check_sync;

  const BcvArgs* bcv() const { return bcv_on ? &bcv_args : nullptr; }  // null: empty selection
  void sync() const { CFD_HIP(hipStreamSynchronize(stream)); }
  void check_launch(const char* where) const { cfd2::check_launch(stream, check_sync, where); }
  void scalar_check(int f) const { scalar_index_check(nf, f); }
};

}  // namespace cfd2
