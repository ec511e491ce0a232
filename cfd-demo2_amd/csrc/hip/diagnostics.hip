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

constexpr uint32_t kBlockCells = 4 * kRedChunkCells;  // one block: 4 chunks of 256 cells

// The blocks are remapped per XCD (xcd_block): XCD k sweeps a contiguous range
// of cells, so the u[other] gathers hit its L2.  Order only.
// Thread t of block b handles cells b*1024 + q*256 + t, q = 0..3 (every load of
// a face slot is one coalesced wavefront access): chunk q of the block is its
// 256 cells of round q, wavefront w the chunk's quarter w.  Sums: the
// quarter's shuffle tree, the chunk's 4 quarters pairwise, then the block's
// units of U chunks -- the tree of k_evolution_partial.  Maxima as bit
// patterns (non-negative values order as unsigned integers; a NaN counts 0).
template <bool FIELDS, bool FORCE>
__global__ void __launch_bounds__(kBlock) k_flow_diag(FlowDiagArgs a) {
  __shared__ double lsum[kFlowDiagSums][4][4];  // [sum][chunk q][quarter w]
  __shared__ unsigned long long lmax[3][4];
  const uint32_t N = a.N;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const uint32_t lb = xcd_block();
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long ms = 0, mo = 0, md = 0;
  for (uint32_t q = 0; q < 4; ++q) {
    const uint64_t ci = (uint64_t)lb * kBlockCells + q * kRedChunkCells + threadIdx.x;
    double t[kFlowDiagSums];
#pragma unroll
    for (int f = 0; f < kFlowDiagSums; ++f) t[f] = 0.0;
    if (ci < N) {
      const uint32_t i = (uint32_t)ci;
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
      const uint32_t nf = fs.nface[i];
      for (uint32_t k = 0; k < nf; ++k) {
        const size_t e = (size_t)k * N + i;
        const uint32_t meta = fs.meta[e];
        const int32_t other = fs.other[e];
        const uint32_t bt = meta & kMetaBtypeMask;
        const float area = fs.area[e];
        const float nx = fs.nx[e], ny = fs.ny[e];  // oriented out of this cell
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
        gux += vfu * nx * area;
        guy += vfu * ny * area;
        gvx += vfv * nx * area;
        gvy += vfv * ny * area;
        if constexpr (FORCE) {
          if ((mask >> k) & 1u) {  // a selected wall face: pressure p_i, diffusion viscosity * area / dist_e
            const double ad = (double)area, dist = (double)fs.dist_e[e];
            fpx += (double)pc * (double)nx * ad;
            fpy += (double)pc * (double)ny * ad;
            fvx += (double)c.viscosity * (double)uc.x * ad / dist;
            fvy += (double)c.viscosity * (double)uc.y * ad / dist;
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
    }
    constexpr int nsum = FORCE ? kFlowDiagSums : 2;  // no region: the force sums are +0
#pragma unroll
    for (int f = 0; f < nsum; ++f) {
      const double r = wave_tree(t[f]);
      if (lane == 0) lsum[f][q][w] = r;
    }
    if constexpr (!FORCE) {
      if (lane == 0) {
#pragma unroll
        for (int f = 2; f < kFlowDiagSums; ++f) lsum[f][q][w] = 0.0;
      }
    }
  }
  ms = wave_max(ms);
  mo = wave_max(mo);
  md = wave_max(md);
  if (lane == 0) {
    lmax[0][w] = ms;
    lmax[1][w] = mo;
    lmax[2][w] = md;
  }
  __syncthreads();
  const uint32_t U = a.U, UB = 4 / U;
  if (threadIdx.x < kFlowDiagSums * UB) {
    const uint32_t f = threadIdx.x / UB, u = threadIdx.x % UB, unit = lb * UB + u;
    double ch[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ch[q] = (lsum[f][q][0] + lsum[f][q][1]) + (lsum[f][q][2] + lsum[f][q][3]);
    const double v = U == 4 ? (ch[0] + ch[1]) + (ch[2] + ch[3]) : (U == 2 ? ch[2 * u] + ch[2 * u + 1] : ch[u]);
    if ((uint64_t)unit * U * kRedChunkCells < N && unit < a.np) a.partial[(size_t)f * a.np + unit] = v;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 67) {
    const uint32_t j = threadIdx.x - 64;
    const unsigned long long m01 = lmax[j][0] > lmax[j][1] ? lmax[j][0] : lmax[j][1];
    const unsigned long long m23 = lmax[j][2] > lmax[j][3] ? lmax[j][2] : lmax[j][3];
    a.blockmax[3 * (size_t)lb + j] = m01 > m23 ? m01 : m23;
  }
}

// folds the per-block maxima: out[j] = max over blocks of blockmax[3 b + j]
__global__ void __launch_bounds__(kBlock) k_flow_diag_max(const unsigned long long* __restrict__ blockmax,
                                                          uint32_t nb, unsigned long long* out) {
  __shared__ unsigned long long lmax[3][4];
  unsigned long long m[3] = {0, 0, 0};
  for (uint32_t b = threadIdx.x; b < nb; b += kBlock) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned long long v = blockmax[3 * (size_t)b + j];
      m[j] = v > m[j] ? v : m[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    m[j] = wave_max(m[j]);
    if ((threadIdx.x & 63) == 0) lmax[j][threadIdx.x >> 6] = m[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint32_t j = threadIdx.x;
    const unsigned long long m01 = lmax[j][0] > lmax[j][1] ? lmax[j][0] : lmax[j][1];
    const unsigned long long m23 = lmax[j][2] > lmax[j][3] ? lmax[j][2] : lmax[j][3];
    out[j] = m01 > m23 ? m01 : m23;
  }
}

}  // namespace

uint32_t flow_diag_blocks(uint32_t N) { return (uint32_t)(((uint64_t)N + kBlockCells - 1) / kBlockCells); }

void launch_flow_diag(const FlowDiagArgs& a, unsigned long long* maxout, hipStream_t s) {
  const uint32_t nb = flow_diag_blocks(a.N);
  if (nb) {
    const bool fields = a.omega_out != nullptr, force = a.wall_mask != nullptr;
    const dim3 g(nb), b(kBlock);
    if (fields && force)
      hipLaunchKernelGGL((k_flow_diag<true, true>), g, b, 0, s, a);
    else if (fields)
      hipLaunchKernelGGL((k_flow_diag<true, false>), g, b, 0, s, a);
    else if (force)
      hipLaunchKernelGGL((k_flow_diag<false, true>), g, b, 0, s, a);
    else
      hipLaunchKernelGGL((k_flow_diag<false, false>), g, b, 0, s, a);
  }
  hipLaunchKernelGGL(k_flow_diag_max, dim3(1), dim3(kBlock), 0, s, a.blockmax, nb, maxout);
}

}  // namespace cfd2
