// Passive scalar transport (kernels.hpp "scalar.hip"): the face-slot assembly
// of one field's implicit-Euler upwind system from the mass fluxes k_prepare
// left in flux_s, one Jacobi sweep over its slot-major ELL image, and the
// read-only field statistics.  Nothing the step reads is written.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

constexpr uint32_t kStatCells = 4 * kRedChunkCells;  // k_scalar_stats: one block, 4 chunks of 256 cells
constexpr uint32_t kDeltaNaN = 0x7f800000u;          // a NaN difference counts as +inf

// Thread per cell (row_id: blocks remapped per XCD), every slot load one
// coalesced wavefront access.
__global__ void __launch_bounds__(kBlock) k_scalar_assemble(ScalarAssembleArgs a) {
  const uint32_t i = row_id();
  const uint32_t N = a.N;
  if (i >= N) return;
  const FaceSlots fs = a.fs;
  const float a_t = a.vol[i] * a.density / a.dt;
  const float rd = a.density * a.diffusivity;
  float diag = a_t;
  float b = a_t * a.phi_old[i];
  const uint32_t nf = fs.nface[i];
  for (uint32_t k = 0; k < nf; ++k) {
    const size_t e = (size_t)k * N + i;
    const uint32_t bt = fs.meta[e] & kMetaBtypeMask;
    const bool internal = fs.other[e] != kNoCell;
    float c = 0.0f;  // wall: zero flux; outlet: zero gradient, flux >= 0 by construction
    if (internal || bt == 1u) {
      const float F = a.flux_s[e];  // mass flux out of this cell
      // the order is fixed (tests/scalar_ref.py restates it): diff = (density *
      // D) * area / dist_e, cin = max(-F, 0), c = cin + diff
      const float diff = rd * fs.area[e] / fs.dist_e[e];
      const float cin = F < 0.0f ? -F : 0.0f;
      c = cin + diff;
    }
    a.coef[(size_t)k * a.ld + i] = c;
    diag += c;
    if (!internal && bt == 1u) b += c * a.inlet_value;
  }
  a.diag[i] = diag;
  a.b[i] = b;
}

__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = w < v ? w : v;
  }
  return v;
}

// One Jacobi sweep, thread per cell.  The slots are taken four at a time: the
// four column / coefficient loads, then the four gathers, are in flight
// together; the sum itself stays left to right in slot order from b_i.
// DELTA: also the block's maximum of |phi_out - phi_in| as a bit pattern.
template <bool DELTA>
__global__ void __launch_bounds__(kBlock) k_scalar_sweep(ScalarSweepArgs a) {
  __shared__ uint32_t lmax[kBlock / 64];
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  const uint32_t i = lb * kBlock + threadIdx.x;
  uint32_t bits = 0;
  if (i < N) {
    float s = a.b[i];
    const float dg = a.diag[i];
    const uint32_t nf = a.nface[i];
    for (uint32_t k0 = 0; k0 < nf; k0 += 4) {
      int32_t o[4];
      float c[4], p[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = k0 + j;
        const bool on = k < nf;
        o[j] = on ? a.other[(size_t)k * N + i] : kNoCell;
        c[j] = on ? a.coef[(size_t)k * a.ld + i] : 0.0f;
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) p[j] = o[j] != kNoCell ? a.phi_in[o[j]] : 0.0f;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
        if (o[j] != kNoCell) s += c[j] * p[j];  // boundary slots are skipped
    }
    const float v = s / dg;
    a.phi_out[i] = v;
    if constexpr (DELTA) {
      const float d = fabsf(v - a.phi_in[i]);
      bits = d == d ? __float_as_uint(d) : kDeltaNaN;
    }
  }
  if constexpr (DELTA) {
    bits = wave_max32(bits);
    if ((threadIdx.x & 63) == 0) lmax[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t m01 = lmax[0] > lmax[1] ? lmax[0] : lmax[1];
      const uint32_t m23 = lmax[2] > lmax[3] ? lmax[2] : lmax[3];
      a.blockmax[lb] = m01 > m23 ? m01 : m23;
    }
  }
}

// folds per-block values: out[j] = min (j < nmin) or max over blocks of v[nv b + j]
__global__ void __launch_bounds__(kBlock) k_scalar_fold(const uint32_t* __restrict__ v, uint32_t nb, uint32_t nv,
                                                        uint32_t nmin, uint32_t* out) {
  __shared__ uint32_t l[kBlock / 64];
  for (uint32_t j = 0; j < nv; ++j) {
    const bool mn = j < nmin;
    uint32_t m = mn ? ~0u : 0u;
    for (uint32_t b = threadIdx.x; b < nb; b += kBlock) {
      const uint32_t x = v[(size_t)nv * b + j];
      m = mn ? (x < m ? x : m) : (x > m ? x : m);
    }
    m = mn ? wave_min32(m) : wave_max32(m);
    if ((threadIdx.x & 63) == 0) l[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t r = l[0];
      for (uint32_t w = 1; w < kBlock / 64; ++w) r = mn ? (l[w] < r ? l[w] : r) : (l[w] > r ? l[w] : r);
      out[j] = r;
    }
    __syncthreads();
  }
}

// Field statistics, the shape of k_flow_diag: thread t of block b handles cells
// b*1024 + q*256 + t, q = 0..3; the sum's tree is the quarter's shuffle tree,
// the chunk's 4 quarters pairwise, then the block's units of U chunks.
__global__ void __launch_bounds__(kBlock) k_scalar_stats(ScalarStatsArgs a) {
  __shared__ double lsum[4][4];  // [chunk q][quarter w]
  __shared__ uint32_t lmm[2][4];
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t kmin = ~0u, kmax = 0u;
  for (uint32_t q = 0; q < 4; ++q) {
    const uint64_t ci = (uint64_t)lb * kStatCells + q * kRedChunkCells + threadIdx.x;
    double t = 0.0;
    if (ci < N) {
      const float ph = a.phi[ci];
      t = (double)a.vol[ci] * (double)ph;
      if (ph == ph) {
        const uint32_t key = scalar_value_key(__float_as_uint(ph));
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
    }
    const double r = wave_tree(t);
    if (lane == 0) lsum[q][w] = r;
  }
  kmin = wave_min32(kmin);
  kmax = wave_max32(kmax);
  if (lane == 0) {
    lmm[0][w] = kmin;
    lmm[1][w] = kmax;
  }
  __syncthreads();
  const uint32_t U = a.U, UB = 4 / U;
  if (threadIdx.x < UB) {
    const uint32_t u = threadIdx.x, unit = lb * UB + u;
    double ch[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ch[q] = (lsum[q][0] + lsum[q][1]) + (lsum[q][2] + lsum[q][3]);
    const double v = unit_value(ch, U, u);
    if ((uint64_t)unit * U * kRedChunkCells < N && unit < a.np) a.partial[unit] = v;
  }
  if (threadIdx.x == 64) {
    uint32_t mn = lmm[0][0], mx = lmm[1][0];
    for (int j = 1; j < 4; ++j) {
      mn = lmm[0][j] < mn ? lmm[0][j] : mn;
      mx = lmm[1][j] > mx ? lmm[1][j] : mx;
    }
    a.blockmm[2 * (size_t)lb] = mn;
    a.blockmm[2 * (size_t)lb + 1] = mx;
  }
}

}  // namespace

uint32_t scalar_sweep_blocks(uint32_t N) { return grid_for(N); }

void launch_scalar_assemble(const ScalarAssembleArgs& a, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_scalar_assemble, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a);
}

void launch_scalar_sweep(const ScalarSweepArgs& a, uint32_t* delta, hipStream_t s) {
  const uint32_t nb = scalar_sweep_blocks(a.N);
  if (nb) {
    if (delta)
      hipLaunchKernelGGL((k_scalar_sweep<true>), dim3(nb), dim3(kBlock), 0, s, a);
    else
      hipLaunchKernelGGL((k_scalar_sweep<false>), dim3(nb), dim3(kBlock), 0, s, a);
  }
  if (delta) hipLaunchKernelGGL(k_scalar_fold, dim3(1), dim3(kBlock), 0, s, a.blockmax, nb, 1u, 0u, delta);
}

void launch_scalar_stats(const ScalarStatsArgs& a, uint32_t* mm, hipStream_t s) {
  const uint32_t nb = flow_diag_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_scalar_stats, dim3(nb), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(k_scalar_fold, dim3(1), dim3(kBlock), 0, s, a.blockmm, nb, 2u, 1u, mm);
}

}  // namespace cfd2
