// What an opt-in feature (the post-processing modules of modules.hpp, Scalars,
// BoundaryVelocity, Viscosity, Penalty) may read of the solver: one value, built fresh by
// Solver::view for every call (the ring rotates), of const members and
// pointers to const.  A method of theirs takes it first and has no other way
// to the solver's state.
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

// The work space of a read-only diagnostic with ns f64 cell sums (one GPU):
// the unit partials and the ns totals, null before the first use.
struct SumBuf {
  double* partial = nullptr;  // [ns * pstride]
  double* res = nullptr;      // [ns]
};
// The geometry of the canonical reductions on one GPU (kernels.hpp RedGeom):
// where a kernel leaves its unit partials and what the finishing kernels read.
struct CellSums {
  uint32_t U;        // chunks per unit (RedGeom::U)
  uint32_t G;        // units per segment
  uint32_t nseg;
  uint32_t pstride;  // unit partials per vector
  uint32_t nunits;
  SumOut out(double* partial) const { return SumOut{U, pstride, partial}; }
  // the source of nvec reductions of unit partials part[v * pstride + k]
  template <class T>
  RedSrcT<T> src(const T* part, int nvec) const {
    return RedSrcT<T>{part, pstride, nunits, G, nseg, (uint32_t)nvec};
  }
  // allocates b in `a` at its first use; the destination of the kernel's sums
  SumOut buf(SumBuf& b, int ns, DeviceArena& a) const {
    if (!b.partial) {
      b.partial = a.alloc<double>((size_t)ns * pstride);
      b.res = a.alloc<double>(ns);
    }
    return out(b.partial);
  }
};

static_assert(kTimeStatsMaxFields == 4, "FlowView::field is written out for four scalar fields");

struct FlowView {
  const int device;
  const hipStream_t stream;
  const bool dist;                // a distributed handle: from Solver::view(nullptr) alone
  const uint32_t N, NG;           // cells of this handle (one GPU: all of them) and of the whole mesh
  const uint32_t ld;              // the slot stride of a per-cell system (Topology::ld)
  const FaceSlots fs;
  const float* const vol;         // [N]
  const float* const flux_s;      // [fs.wf * N] the face-slot fluxes as the last prepare left them
  const CellSums sums;
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
  const float* const visc_mu;     // [N] the viscosity per cell (viscosity.hpp), or null: constants.viscosity
  const uint64_t surface_gen;     // grows with every change of the scalar or boundary-velocity configuration
  const bool check_sync;
  // nf, field, bcv_args and bcv_on are copies for the post-processing modules.
  // Scalars and BoundaryVelocity read their own members, never these: phi
  // swaps with its partner during an advance, and the copy would be stale.

  const BcvArgs* bcv() const { return bcv_on ? &bcv_args : nullptr; }  // null: empty selection
  void sync() const { CFD_HIP(hipStreamSynchronize(stream)); }
  void check_launch(const char* where) const { cfd2::check_launch(stream, check_sync, where); }
  void scalar_check(int f) const { scalar_index_check(nf, f); }
  // finishes the ns totals of b and reads them back into h[0, ns)
  void sum_read(const SumBuf& b, int ns, double* h, const char* where) const {
    launch_evolution_final(sums.src(b.partial, ns), b.res, stream);
    check_launch(where);
    CFD_HIP(hipMemcpyAsync(h, b.res, ns * sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
  }
};

}  // namespace cfd2
