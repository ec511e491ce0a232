// Viscosity models (include/cfd2_amd.h "Arithmetic of the viscosity models" is
// the contract; kernels.hpp "viscosity.hip"): k_viscosity_model, one read-only
// face-slot sweep over the cells of the current state, one thread per cell,
// slot-major coalesced loads, the blocks remapped per XCD as in k_flow_diag.
// It forms the Green-Gauss gradients of the current u exactly as prepare_cell
// does (not the stale grad_u / grad_v buffers: mu is a function of the state
// alone), the shear rate in f32, the model in f64 through pow_det, and stores
// mu[i] and the shear rate.  Minimum and maximum of mu (positive floats order
// as their bit patterns) and the counts of clamped cells are reduced per
// wavefront and folded with integer atomics: order-independent.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "pow_det.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// BCV: the form with prescribed boundary velocities, the face value of prepare_cell<true>.
template <bool BCV>
__device__ __forceinline__ void viscosity_model_cell(const ViscosityModelArgs& a, const BcvArgs& v) {
  const uint32_t N = a.N;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const uint32_t i = row_id();
  const bool live = i < N;
  uint32_t bmin = 0xFFFFFFFFu, bmax = 0u;
  bool below = false, above = false;
  if (live) {
    const float vol = a.vol[i];
    const float2 uc = a.u[i];
    float gux = 0.0f, guy = 0.0f, gvx = 0.0f, gvy = 0.0f;
    const uint32_t nf = fs.nface[i];
    uint32_t brow = 0;
    if constexpr (BCV) brow = v.sel[i];
    for (uint32_t k = 0; k < nf; ++k) {
      const size_t e = (size_t)k * N + i;
      const uint32_t meta = fs.meta[e];
      const int32_t other = fs.other[e];
      const uint32_t bt = meta & kMetaBtypeMask;
      const float area = fs.area[e];
      const float nx = fs.nx[e], ny = fs.ny[e];  // oriented out of this cell
      // face value of u per face type: prepare_cell's branch (flux.hip), as k_flow_diag carries it
      float vfu, vfv;
      if (other != kNoCell) {
        const float2 uo = a.u[other];
        const float lp = fs.lam_s[e];
        if ((meta & kMetaDegen) == 0) {
          vfu = lp * uc.x + (1.0f - lp) * uo.x;
          vfv = lp * uc.y + (1.0f - lp) * uo.y;
        } else {
          vfu = 0.5f * (uc.x + uo.x);
          vfv = 0.5f * (uc.y + uo.y);
        }
      } else if (bt == 1u) {
        const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
        vfu = c.inlet_velocity * ramp;
        vfv = 0.0f;
      } else if (bt == 3u) {
        vfu = 0.0f;
        vfv = 0.0f;
      } else {
        vfu = uc.x;
        vfv = uc.y;
      }
      if constexpr (BCV) {
        if (other == kNoCell && brow != 0u) {
          const float4 t = v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
          if (t.z != 0.0f) {
            const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
            const float g = (bt == 1u ? v.inlet_scale : v.wall_scale) * ramp;
            vfu = t.x * g;
            vfv = t.y * g;
          }
        }
      }
      gux += vfu * nx * area;
      guy += vfu * ny * area;
      gvx += vfv * nx * area;
      gvy += vfv * ny * area;
    }
    const float ux = gux / vol, uy = guy / vol, vx = gvx / vol, vy = gvy / vol;
    const float sh = uy + vx;
    const float gdot = sqrtf(2.0f * (ux * ux) + 2.0f * (vy * vy) + sh * sh);
    const cfd_viscosity_model& md = a.model;
    const double g = (double)gdot;
    double m;
    if (md.kind == 1) {
      const double gm = (double)md.gamma_min;
      m = (double)md.K * pow_det(g > gm ? g : gm, (double)md.n - 1.0);
    } else {
      const double lg = (double)md.lambda * g;
      m = (double)md.mu_inf + ((double)md.mu0 - (double)md.mu_inf) * pow_det(1.0 + lg * lg, ((double)md.n - 1.0) / 2.0);
    }
    const double lo = (double)md.mu_min, hi = (double)md.mu_max;
    below = m < lo;
    above = m > hi;
    if (below) m = lo;
    if (above) m = hi;
    const float mu = (float)m;
    a.mu[i] = mu;
    a.gdot[i] = gdot;
    bmin = bmax = __float_as_uint(mu);
  }
  bmin = wave_min(bmin);
  bmax = wave_max(bmax);
  const uint32_t nb = (uint32_t)__popcll(__ballot(below)), na = (uint32_t)__popcll(__ballot(above));
  if ((threadIdx.x & 63u) == 0u) {
    atomicMin(a.stats + 0, bmin);
    atomicMax(a.stats + 1, bmax);
    if (nb) atomicAdd(a.stats + 2, nb);
    if (na) atomicAdd(a.stats + 3, na);
  }
}

__global__ void __launch_bounds__(kBlock) k_viscosity_model(ViscosityModelArgs a) {
  viscosity_model_cell<false>(a, BcvArgs{});
}
__global__ void __launch_bounds__(kBlock) k_viscosity_model_bcv(ViscosityModelArgs a, BcvArgs v) {
  viscosity_model_cell<true>(a, v);
}

}  // namespace

void launch_viscosity_model(const ViscosityModelArgs& a, const BcvArgs* v, hipStream_t s) {
  if (!a.N) return;
  const dim3 g(grid_for(a.N)), b(kBlock);
  if (v)
    hipLaunchKernelGGL(k_viscosity_model_bcv, g, b, 0, s, a, *v);
  else
    hipLaunchKernelGGL(k_viscosity_model, g, b, 0, s, a);
}

}  // namespace cfd2
