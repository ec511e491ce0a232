// Time statistics and the monitor history (include/cfd2_amd.h "Arithmetic of
// the time statistics" is the contract; kernels.hpp "timestats.hip").
//
// k_tstats: one pass over the cells, the weighted incremental (West / Welford)
// update of every enabled plane in f64, one rounding per operation (the build
// passes -ffp-contract=off).  A lane owns two consecutive cells: one 16-byte
// read of u, 8-byte reads of p and of every field, and per plane one 16-byte
// read and one 16-byte store (the planes' stride is even, so every pair is
// 16-byte aligned).  The odd last cell runs the same update on one cell with
// 8-byte plane accesses.  No LDS, no atomics, no reduction: a cell's result
// depends on that cell's planes and sample only.  The planes are read once per
// call and are far larger than the Infinity Cache at the sizes that matter, so
// their loads are nontemporal (device_util.hpp ldx): they do not displace the
// state the next step reads.
//
// k_monitor_record: one lane per probe; lane 0 of block 0 also writes the
// slot's time and dt, lanes 0..8 of block 0 the nine words of the flow
// diagnostics' device result.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// Dev / mean_update / m2_update, the update of one quantity: device_util.hpp

// V = double2 (two cells) or double (one): every plane access of a lane
template <class V>
struct Acc;
template <>
struct Acc<double2> {
  static constexpr int n = 2;
  static __device__ __forceinline__ double& at(double2& v, int k) { return k == 0 ? v.x : v.y; }
};
template <>
struct Acc<double> {
  static constexpr int n = 1;
  static __device__ __forceinline__ double& at(double& v, int) { return v; }
};

// Cells [i, i + n) of every plane; x[q][k]: quantity q (u, v, p) of cell k.
template <bool M2, bool FIELDS, class V>
__device__ __forceinline__ void tstats_cells(const TimeStatsArgs& a, uint32_t i, const float (&xu)[2], const float (&xv)[2],
                                              const float (&xp)[2]) {
  constexpr int n = Acc<V>::n;
  const double w = a.w, r = a.r;
  const size_t ld = a.ld;
  double* base = a.planes + i;
  auto plane = [&](uint32_t q) { return reinterpret_cast<V*>(base + (size_t)q * ld); };
  V mu = ldx<true>(plane(0)), mv = ldx<true>(plane(1)), mp = ldx<true>(plane(2));
  Dev du[n], dv[n], dp[n];
#pragma unroll
  for (int k = 0; k < n; ++k) {
    du[k] = mean_update((double)xu[k], r, Acc<V>::at(mu, k));
    dv[k] = mean_update((double)xv[k], r, Acc<V>::at(mv, k));
    dp[k] = mean_update((double)xp[k], r, Acc<V>::at(mp, k));
  }
  *plane(0) = mu;
  *plane(1) = mv;
  *plane(2) = mp;
  double wdu[n], wdv[n];
#pragma unroll
  for (int k = 0; k < n; ++k) {
    wdu[k] = w * du[k].d;
    wdv[k] = w * dv[k].d;
  }
  uint32_t q = 3;
  if constexpr (M2) {
    V uu = ldx<true>(plane(3)), uv = ldx<true>(plane(4)), vv = ldx<true>(plane(5)), pp = ldx<true>(plane(6));
#pragma unroll
    for (int k = 0; k < n; ++k) {
      Acc<V>::at(uu, k) += wdu[k] * du[k].e;
      Acc<V>::at(uv, k) += wdu[k] * dv[k].e;
      Acc<V>::at(vv, k) += wdv[k] * dv[k].e;
      m2_update(w, dp[k], dp[k].e, Acc<V>::at(pp, k));
    }
    *plane(3) = uu;
    *plane(4) = uv;
    *plane(5) = vv;
    *plane(6) = pp;
    q = 7;
  }
  if constexpr (FIELDS) {
#pragma unroll
    for (uint32_t f = 0; f < kTimeStatsMaxFields; ++f) {  // unrolled: phi[f] is a kernel argument, not an indexed array
      if (f >= a.nf) break;                               // uniform
      const float* phi = a.phi[f] + i;
      float xf[n];
      if constexpr (n == 2) {
        const float2 t = ldx<false>(reinterpret_cast<const float2*>(phi));
        xf[0] = t.x, xf[1] = t.y;
      } else {
        xf[0] = ldx<false>(phi);
      }
      V mf = ldx<true>(plane(q)), ff = ldx<true>(plane(q + 1));
      Dev df[n];
#pragma unroll
      for (int k = 0; k < n; ++k) {
        df[k] = mean_update((double)xf[k], r, Acc<V>::at(mf, k));
        m2_update(w, df[k], df[k].e, Acc<V>::at(ff, k));
      }
      *plane(q) = mf;
      *plane(q + 1) = ff;
      q += 2;
      if constexpr (M2) {
        V uf = ldx<true>(plane(q)), vf = ldx<true>(plane(q + 1));
#pragma unroll
        for (int k = 0; k < n; ++k) {
          Acc<V>::at(uf, k) += wdu[k] * df[k].e;
          Acc<V>::at(vf, k) += wdv[k] * df[k].e;
        }
        *plane(q) = uf;
        *plane(q + 1) = vf;
        q += 2;
      }
    }
  }
}

template <bool M2, bool FIELDS>
__global__ void __launch_bounds__(kBlock) k_tstats(TimeStatsArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t i0 = 2 * t;
  if (i0 >= a.N) return;
  const uint32_t i = (uint32_t)i0;
  if (i + 1u < a.N) {
    const float4 u2 = ldx<false>(reinterpret_cast<const float4*>(a.u + i));  // (u, v) of cells i and i + 1
    const float2 p2 = ldx<false>(reinterpret_cast<const float2*>(a.p + i));
    const float xu[2] = {u2.x, u2.z}, xv[2] = {u2.y, u2.w}, xp[2] = {p2.x, p2.y};
    tstats_cells<M2, FIELDS, double2>(a, i, xu, xv, xp);
  } else {  // the odd last cell
    const float2 u1 = ldx<false>(a.u + i);
    const float xu[2] = {u1.x, 0.0f}, xv[2] = {u1.y, 0.0f}, xp[2] = {ldx<false>(a.p + i), 0.0f};
    tstats_cells<M2, FIELDS, double>(a, i, xu, xv, xp);
  }
}

__global__ void __launch_bounds__(kBlock) k_monitor_record(MonitorRecordArgs a) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t == 0) {
    a.time_out[0] = a.time;
    a.time_out[1] = a.dt;
  }
  if (a.diag_out && t < kMonitorDiagWords) a.diag_out[t] = a.diag_res[t];
  if (t >= a.P) return;
  const uint32_t c = a.cells[t];  // < N: checked when the monitor was enabled
  const uint32_t stride = 3u + a.ns;
  float* out = a.probe_out + (size_t)t * stride;
  const float2 u = a.u[c];
  out[0] = u.x;
  out[1] = u.y;
  out[2] = a.p[c];
#pragma unroll
  for (uint32_t f = 0; f < kTimeStatsMaxFields; ++f)
    if (f < a.ns) out[3 + f] = a.phi[f][c];
}

}  // namespace

void launch_tstats(const TimeStatsArgs& a, bool second_moments, hipStream_t s) {
  if (a.N == 0) return;
  const dim3 g(grid_for(((size_t)a.N + 1) / 2)), b(kBlock);
  const bool fields = a.nf != 0;
  if (second_moments && fields)
    hipLaunchKernelGGL((k_tstats<true, true>), g, b, 0, s, a);
  else if (second_moments)
    hipLaunchKernelGGL((k_tstats<true, false>), g, b, 0, s, a);
  else if (fields)
    hipLaunchKernelGGL((k_tstats<false, true>), g, b, 0, s, a);
  else
    hipLaunchKernelGGL((k_tstats<false, false>), g, b, 0, s, a);
}

void launch_monitor_record(const MonitorRecordArgs& a, hipStream_t s) {
  const unsigned g = std::max(1u, grid_for(a.P));
  hipLaunchKernelGGL(k_monitor_record, dim3(g), dim3(kBlock), 0, s, a);
}

}  // namespace cfd2
