// Flow diagnostics: one read-only face-slot sweep over the owned cells of the
// current state (k_flow_diag) -- Green-Gauss velocity gradients exactly as
// k_prepare forms them, from which vorticity and divergence per cell, their
// maxima, the maximum of |u|^2, and six f64 sums (kinetic energy, enstrophy,
// pressure and viscous force on the selected wall faces) in the canonical
// reduction order (kernels.hpp).  Nothing the step reads is written.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// The blocks are remapped per XCD (xcd_block): XCD k sweeps a contiguous range
// of cells, so the u[other] gathers hit its L2.  Order only.
// A block takes kRedBlockCells cells (every load of a face slot is one
// coalesced wavefront access); the sums run over the shared skeleton
// (reduce_dev.hpp sum_accumulate / sum_store) -- the tree of
// k_evolution_partial.  Without a force region only the first two sums are
// reduced; the force sums are +0.  Maxima as bit patterns (non-negative values
// order as unsigned integers; a NaN counts 0).
// BCV: the form with prescribed boundary velocities (kernels.hpp BcvArgs): the
// face value follows prepare_cell<true>, the viscous force of a selected wall
// slot takes u - ub.
// VISC: the form with a viscosity per cell: the viscous force of a wall slot
// takes mu[i] for c.viscosity (one more coalesced 4-byte load per cell).  Only
// the FORCE instances have it: nothing else here reads the viscosity.
template <bool FIELDS, bool FORCE, bool BCV, bool VISC = false>
__device__ __forceinline__ void flow_diag_block(const FlowDiagArgs& a, const BcvArgs& v,
                                                const float* __restrict__ mu = nullptr) {
  __shared__ double lsum[kFlowDiagSums][4][4];  // [sum][chunk q][quarter w]
  __shared__ unsigned long long lmax[3][4];
  const uint32_t N = a.N;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const uint32_t lb = xcd_block();
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long ms = 0, mo = 0, md = 0;
  sum_accumulate<kFlowDiagSums, FORCE ? kFlowDiagSums : 2>(lsum, N, lb, [&](uint32_t i, double* t) {
    const float vol = a.vol[i];
    const float2 uc = a.u[i];
    float gux = 0.0f, guy = 0.0f, gvx = 0.0f, gvy = 0.0f;
    double fpx = 0.0, fpy = 0.0, fvx = 0.0, fvy = 0.0;
    uint32_t mask = 0;
    float pc = 0.0f;
    if constexpr (FORCE) {
      mask = a.wall_mask[i];
      pc = a.p[i];
    }
    float visc = c.viscosity;
    if constexpr (VISC) visc = mu[i];
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
      bool bsel = false;  // BCV: a selected slot, its velocity (sbx, sby)
      float sbx = 0.0f, sby = 0.0f;
      if constexpr (BCV) {
        if (other == kNoCell && brow != 0u) {
          const float4 t = v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
          if (t.z != 0.0f) {
            const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
            const float g = (bt == 1u ? v.inlet_scale : v.wall_scale) * ramp;
            bsel = true;
            sbx = t.x * g;
            sby = t.y * g;
          }
        }
      }
      // face value of u per face type: a copy of prepare_cell's branch (flux.hip;
      // prepare_coupled.wgsl:281-324).  One shared function changed k_prepare's
      // register allocation, so the two copies stay, held together by
      // tests/test_gpu_flow_diag.py's k_prepare-bits test.
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
        if (bsel) {
          vfu = sbx;
          vfv = sby;
        }
      }
      gux += vfu * nx * area;
      guy += vfu * ny * area;
      gvx += vfv * nx * area;
      gvy += vfv * ny * area;
      if constexpr (FORCE) {
        if ((mask >> k) & 1u) {  // a selected wall face: pressure p_i, diffusion viscosity * area / dist_e
          const double ad = (double)area, dist = (double)fs.dist_e[e];
          fpx += (double)pc * (double)nx * ad;
          fpy += (double)pc * (double)ny * ad;
          double rux = (double)uc.x, ruy = (double)uc.y;  // relative to the wall
          if constexpr (BCV) {
            if (bsel) {
              rux = (double)uc.x - (double)sbx;
              ruy = (double)uc.y - (double)sby;
            }
          }
          fvx += (double)visc * rux * ad / dist;
          fvy += (double)visc * ruy * ad / dist;
        }
      }
    }
    const float2 gu = make_float2(gux / vol, guy / vol);
    const float2 gv = make_float2(gvx / vol, gvy / vol);
    const float omega = gv.x - gu.y;
    const float dv = gu.x + gv.y;
    if constexpr (FIELDS) {
      a.omega_out[i] = omega;
      a.div_out[i] = dv;
    }
    const double s = (double)uc.x * (double)uc.x + (double)uc.y * (double)uc.y;
    const double od = (double)omega;
    t[0] = 0.5 * (double)vol * s;
    t[1] = 0.5 * (double)vol * od * od;
    t[2] = fpx;
    t[3] = fpy;
    t[4] = fvx;
    t[5] = fvy;
    const unsigned long long bs = s == s ? (unsigned long long)__double_as_longlong(s) : 0ull;
    const float ao = fabsf(omega), ad = fabsf(dv);
    const unsigned long long bo = ao == ao ? (unsigned long long)__float_as_uint(ao) : 0ull;
    const unsigned long long bd = ad == ad ? (unsigned long long)__float_as_uint(ad) : 0ull;
    ms = bs > ms ? bs : ms;
    mo = bo > mo ? bo : mo;
    md = bd > md ? bd : md;
  });
  ms = wave_max(ms);
  mo = wave_max(mo);
  md = wave_max(md);
  if (lane == 0) {
    lmax[0][w] = ms;
    lmax[1][w] = mo;
    lmax[2][w] = md;
  }
  __syncthreads();
  sum_store<kFlowDiagSums>(lsum, a.out, N, lb);
  if (threadIdx.x >= 64 && threadIdx.x < 67) {
    const uint32_t j = threadIdx.x - 64;
    a.blockmax[3 * (size_t)lb + j] = block_of4_max(lmax[j]);
  }
}
template <bool FIELDS, bool FORCE>
__global__ void __launch_bounds__(kBlock) k_flow_diag(FlowDiagArgs a) {
  flow_diag_block<FIELDS, FORCE, false>(a, BcvArgs{});
}
template <bool FIELDS, bool FORCE>
__global__ void __launch_bounds__(kBlock) k_flow_diag_bcv(FlowDiagArgs a, BcvArgs v) {
  flow_diag_block<FIELDS, FORCE, true>(a, v);
}
template <bool FIELDS>
__global__ void __launch_bounds__(kBlock) k_flow_diag_visc(FlowDiagArgs a, const float* __restrict__ mu) {
  flow_diag_block<FIELDS, true, false, true>(a, BcvArgs{}, mu);
}
template <bool FIELDS>
__global__ void __launch_bounds__(kBlock) k_flow_diag_bcv_visc(FlowDiagArgs a, BcvArgs v, const float* __restrict__ mu) {
  flow_diag_block<FIELDS, true, true, true>(a, v, mu);
}

// The wall-motion sums (kernels.hpp WallMotionArgs) over the shared skeleton:
// a cell with a force-region slot walks the set bits of its mask in ascending
// order, every other cell loads that word alone.  Read-only.
__global__ void __launch_bounds__(kBlock) k_wall_motion(WallMotionArgs a) {
  __shared__ double lsum[kWallMotionSums][4][4];  // [sum][chunk q][quarter w]
  const uint32_t N = a.N;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const uint32_t lb = xcd_block();
  sum_accumulate<kWallMotionSums>(lsum, N, lb, [&](uint32_t i, double* t) {
    uint32_t walls = a.wall_mask[i];
    if (walls) {
      const float2 uc = a.u[i];
      const float pc = a.p[i];
      const uint32_t crow = a.crow[i];  // != 0: the host gives every cell of the region a row
      const uint32_t brow = a.v.sel ? a.v.sel[i] : 0u;
      const float visc = a.mu ? a.mu[i] : c.viscosity;  // a viscosity per cell, as k_flow_diag's VISC form
      while (walls && crow) {
        const uint32_t k = (uint32_t)__ffs((int)walls) - 1u;
        walls &= walls - 1u;
        const size_t e = (size_t)k * N + i;
        const double ad = (double)fs.area[e], dist = (double)fs.dist_e[e];
        const float nx = fs.nx[e], ny = fs.ny[e];
        bool bsel = false;
        float sbx = 0.0f, sby = 0.0f;
        if (brow != 0u) {
          const float4 tb = a.v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
          if (tb.z != 0.0f) {
            const float g = a.v.wall_scale * wsmoothstep(0.0f, c.ramp_time, c.time);
            bsel = true;
            sbx = tb.x * g;
            sby = tb.y * g;
          }
        }
        const double fpx = (double)pc * (double)nx * ad;
        const double fpy = (double)pc * (double)ny * ad;
        double rux = (double)uc.x, ruy = (double)uc.y;
        if (bsel) {
          rux = (double)uc.x - (double)sbx;
          ruy = (double)uc.y - (double)sby;
        }
        const double fvx = (double)visc * rux * ad / dist;
        const double fvy = (double)visc * ruy * ad / dist;
        const double2 fc = a.ctr[(size_t)(crow - 1u) * (uint32_t)fs.wf + k];
        const double rx = fc.x - a.x0, ry = fc.y - a.y0;
        t[0] += rx * fpy - ry * fpx;
        t[1] += rx * fvy - ry * fvx;
        if (bsel) t[2] -= (fpx + fvx) * (double)sbx + (fpy + fvy) * (double)sby;
      }
    }
  });
  __syncthreads();
  sum_store<kWallMotionSums>(lsum, a.out, N, lb);
}

}  // namespace

void launch_flow_diag(const FlowDiagArgs& a, const BcvArgs* v, const float* mu, unsigned long long* maxout,
                      hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) {
    const bool fields = a.omega_out != nullptr, force = a.wall_mask != nullptr;
    const dim3 g(nb), b(kBlock);
    auto go = [&](auto plain, auto bcv) {  // the pair of one (FIELDS, FORCE)
      if (v)
        hipLaunchKernelGGL(bcv, g, b, 0, s, a, *v);
      else
        hipLaunchKernelGGL(plain, g, b, 0, s, a);
    };
    auto go_visc = [&](auto plain, auto bcv) {  // the pair of one FIELDS, with a force region
      if (v)
        hipLaunchKernelGGL(bcv, g, b, 0, s, a, *v, mu);
      else
        hipLaunchKernelGGL(plain, g, b, 0, s, a, mu);
    };
    if (mu && force && fields)
      go_visc(k_flow_diag_visc<true>, k_flow_diag_bcv_visc<true>);
    else if (mu && force)
      go_visc(k_flow_diag_visc<false>, k_flow_diag_bcv_visc<false>);
    else if (fields && force)
      go(k_flow_diag<true, true>, k_flow_diag_bcv<true, true>);
    else if (fields)
      go(k_flow_diag<true, false>, k_flow_diag_bcv<true, false>);
    else if (force)
      go(k_flow_diag<false, true>, k_flow_diag_bcv<false, true>);
    else
      go(k_flow_diag<false, false>, k_flow_diag_bcv<false, false>);
  }
  hipLaunchKernelGGL(k_block_fold<unsigned long long>, dim3(1), dim3(kBlock), 0, s, a.blockmax, nb, 3u, 0u, maxout);
}

void launch_wall_motion(const WallMotionArgs& a, hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_wall_motion, dim3(nb), dim3(kBlock), 0, s, a);
}

}  // namespace cfd2
