// Wall surface distributions (include/cfd2_amd.h "Arithmetic of the surface
// channels" is the contract; kernels.hpp "surface.hip").
//
// k_surface_sample / k_surface_accumulate: one thread per face of the compact
// table, 256-thread blocks.  The table read (cell, slot) is coalesced; the
// gathers that depend on it (p, u, the four slot arrays, each field's phi and
// image word) are issued together before any arithmetic.  A surface has
// O(sqrt N) faces: the kernels are latency-bound gathers, so no LDS, no
// atomics, no reduction -- a face's result depends on that face's cell only.
// Every term is f64 from the f32 inputs and repeats, operation for operation,
// the term of the sum it belongs to: k_flow_diag's fpx / fpy / fvx / fvy
// (diagnostics.hip) and k_scalar_wall_flux's t[0] (scalar.hip), so a fold of
// the channels in those kernels' order gives their bits.
// BCV: the form with prescribed boundary velocities (kernels.hpp BcvArgs), the
// pair k_flow_diag / k_flow_diag_bcv is the model: the plain kernels take no
// BcvArgs and read neither the per-cell row index nor the table.
// The accumulate form feeds every channel value into its mean and M2 (the
// weighted West / Welford update shared with timestats.hip) instead of storing
// it: one launch per sample, no intermediate pass.  The running weight W stays
// on the host, as the time statistics keep theirs: w and r = w / (W + w) are
// kernel arguments.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// Face j of the table: emit(channel, value) for every channel in ascending order.
// VISC: the form with a viscosity per cell (one more gather, mu[i], with the
// others): channels 3 and 4 take it for c.viscosity, as k_flow_diag's VISC form.
template <bool BCV, bool VISC, class Emit>
__device__ __forceinline__ void surface_face(const SurfaceArgs& a, const BcvArgs& v, const float* __restrict__ mu,
                                             uint32_t j, Emit&& emit) {
  const uint32_t i = a.cell[j], k = a.slot[j];
  const size_t e = (size_t)k * a.N + i;
  const float pc = a.p[i];
  const float2 uc = a.u[i];
  float visc = a.c.viscosity;
  if constexpr (VISC) visc = mu[i];
  const float area = a.area[e], nx = a.nx[e], ny = a.ny[e], de = a.dist_e[e];
  float ph[kTimeStatsMaxFields];
  uint32_t sw[kTimeStatsMaxFields];
#pragma unroll
  for (uint32_t f = 0; f < kTimeStatsMaxFields; ++f) {  // unrolled: registers, not an indexed array
    ph[f] = 0.0f;
    sw[f] = 0u;
    if (f < a.nf) {  // uniform
      ph[f] = a.f[f].phi[i];
      if (a.f[f].sel) sw[f] = a.f[f].sel[i];
    }
  }
  bool bsel = false;  // BCV: a slot the selection moves, its velocity (sbx, sby)
  float sbx = 0.0f, sby = 0.0f;
  if constexpr (BCV) {
    const uint32_t brow = v.sel[i];
    if (brow != 0u) {
      const float4 t = v.tab[(size_t)(brow - 1u) * a.wf + k];
      if (t.z != 0.0f) {  // a wall slot: every face of the table is one
        const float g = v.wall_scale * wsmoothstep(0.0f, a.c.ramp_time, a.c.time);
        bsel = true;
        sbx = t.x * g;
        sby = t.y * g;
      }
    }
  }
  const double ad = (double)area, dist = (double)de;
  emit(0u, (double)pc);
  emit(1u, (double)pc * (double)nx * ad);
  emit(2u, (double)pc * (double)ny * ad);
  double rux = (double)uc.x, ruy = (double)uc.y;  // relative to the wall
  if constexpr (BCV) {
    if (bsel) {
      rux = (double)uc.x - (double)sbx;
      ruy = (double)uc.y - (double)sby;
    }
  }
  emit(3u, (double)visc * rux * ad / dist);
  emit(4u, (double)visc * ruy * ad / dist);
#pragma unroll
  for (uint32_t f = 0; f < kTimeStatsMaxFields; ++f) {
    if (f >= a.nf) break;  // uniform
    const SurfaceField& sf = a.f[f];
    double flux = 0.0;
    if (k < 31u && ((sw[f] >> k) & 1u) != 0u) {  // bit 31 of the image word marks a source cell
      if (sf.kind == 1)
        flux = (double)scalar_wall_coef(sf.rd, area, de) * ((double)sf.value - (double)ph[f]);
      else
        flux = (double)sf.value * (double)area;
    }
    emit(kSurfaceBaseChannels + 2u * f, flux);
    emit(kSurfaceBaseChannels + 2u * f + 1u, (double)ph[f]);
  }
}

template <bool BCV, bool VISC = false>
__device__ __forceinline__ void surface_sample(const SurfaceArgs& a, const BcvArgs& v,
                                               const float* __restrict__ mu = nullptr) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.n) return;
  double* out = a.out + j;
  const size_t ld = a.ld;
  surface_face<BCV, VISC>(a, v, mu, j, [&](uint32_t ch, double x) { out[(size_t)ch * ld] = x; });
}

template <bool BCV, bool VISC = false>
__device__ __forceinline__ void surface_accumulate(const SurfaceArgs& a, const BcvArgs& v,
                                                   const float* __restrict__ mu = nullptr) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.n) return;
  double* mean = a.mean + j;
  double* m2 = a.m2 + j;
  const size_t ld = a.ld;
  const double w = a.w, r = a.r;
  surface_face<BCV, VISC>(a, v, mu, j, [&](uint32_t ch, double x) {
    const size_t o = (size_t)ch * ld;
    double m = mean[o], M = m2[o];
    const Dev q = mean_update(x, r, m);
    m2_update(w, q, q.e, M);
    mean[o] = m;
    m2[o] = M;
  });
}

__global__ void __launch_bounds__(kBlock) k_surface_sample(SurfaceArgs a) { surface_sample<false>(a, BcvArgs{}); }
__global__ void __launch_bounds__(kBlock) k_surface_sample_bcv(SurfaceArgs a, BcvArgs v) { surface_sample<true>(a, v); }
__global__ void __launch_bounds__(kBlock) k_surface_accumulate(SurfaceArgs a) {
  surface_accumulate<false>(a, BcvArgs{});
}
__global__ void __launch_bounds__(kBlock) k_surface_accumulate_bcv(SurfaceArgs a, BcvArgs v) {
  surface_accumulate<true>(a, v);
}
__global__ void __launch_bounds__(kBlock) k_surface_sample_visc(SurfaceArgs a, const float* __restrict__ mu) {
  surface_sample<false, true>(a, BcvArgs{}, mu);
}
__global__ void __launch_bounds__(kBlock) k_surface_sample_bcv_visc(SurfaceArgs a, BcvArgs v,
                                                                    const float* __restrict__ mu) {
  surface_sample<true, true>(a, v, mu);
}
__global__ void __launch_bounds__(kBlock) k_surface_accumulate_visc(SurfaceArgs a, const float* __restrict__ mu) {
  surface_accumulate<false, true>(a, BcvArgs{}, mu);
}
__global__ void __launch_bounds__(kBlock) k_surface_accumulate_bcv_visc(SurfaceArgs a, BcvArgs v,
                                                                        const float* __restrict__ mu) {
  surface_accumulate<true, true>(a, v, mu);
}

}  // namespace

void launch_surface_sample(const SurfaceArgs& a, const BcvArgs* v, const float* mu, hipStream_t s) {
  if (a.n == 0) return;
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (mu && v)
    hipLaunchKernelGGL(k_surface_sample_bcv_visc, g, b, 0, s, a, *v, mu);
  else if (mu)
    hipLaunchKernelGGL(k_surface_sample_visc, g, b, 0, s, a, mu);
  else if (v)
    hipLaunchKernelGGL(k_surface_sample_bcv, g, b, 0, s, a, *v);
  else
    hipLaunchKernelGGL(k_surface_sample, g, b, 0, s, a);
}

void launch_surface_accumulate(const SurfaceArgs& a, const BcvArgs* v, const float* mu, hipStream_t s) {
  if (a.n == 0) return;
  const dim3 g(grid_for(a.n)), b(kBlock);
  if (mu && v)
    hipLaunchKernelGGL(k_surface_accumulate_bcv_visc, g, b, 0, s, a, *v, mu);
  else if (mu)
    hipLaunchKernelGGL(k_surface_accumulate_visc, g, b, 0, s, a, mu);
  else if (v)
    hipLaunchKernelGGL(k_surface_accumulate_bcv, g, b, 0, s, a, *v);
  else
    hipLaunchKernelGGL(k_surface_accumulate, g, b, 0, s, a);
}

}  // namespace cfd2
