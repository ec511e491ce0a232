// FGMRES: BLAS-1 with the canonical reductions, classical Gram-Schmidt, the
// Givens / triangular steps and the solution update.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// Tuning constants below are plain numbers (A/B-tuned with
// tools/ab_variants.py); every compile-time switch between two code paths
// was removed once its A/B was decided (round 4; git history keeps the losers).
//
// One basis load in flight per wavefront in the CGS kernels (load_cells3 SER)
// on meshes of at least this many cells (per rank); below it, every load of a
// wavefront stays in flight together.  With ~15+ blocks per CU the serialised
// loads win (same-box A/B at C2: update 346 -> 295, dots 294 -> 281 us); with
// ~4 blocks per CU nothing hides a wavefront's one-at-a-time loads (C1: dots
// 41.8 -> 31.0, update 40.5 -> 36.2 us unserialised; profiles/r03/ab_log.md).
#ifndef CFD_CGS_SER_MIN_CELLS
#define CFD_CGS_SER_MIN_CELLS (1u << 22)
#endif

// 3-component cell vectors in the reduction kernels (kernels.hpp: the cell
// term of a dot is (x_u y_u + x_v y_v) + x_p y_p).  Block b covers the 4
// chunks of cells [1024 b, 1024 b + 1024); lane l of wavefront w holds cell
// c_q = 1024 b + 256 q + 64 w + l of chunk q (q = 0..3), its 3 floats by one
// 12-byte access, so the block's 4 wavefronts read one chunk together (768
// contiguous bytes per instruction).  A chunk value is the pairwise tree over
// its 256 cells: each wavefront's 64 (a quarter, wave_tree), then the 4
// quarters (quarter_chunk).  Cells past N: 0.  SER: every load completes
// before the next issues -- for these kernels, which stream up to 51 vectors
// at once, measured faster than keeping a wavefront's loads in flight
// together (same-box A/B at C2: CGS update 349 -> 294 us, dots 300 -> 289).
__device__ __forceinline__ size_t cell_qb(uint32_t b, uint32_t q) {
  return (size_t)b * 1024u + 256u * q + (threadIdx.x & ~63u) + red_lane();
}
template <bool FULL, bool NT = false, bool SER = false>
__device__ __forceinline__ void load_cells3(const float* p, uint32_t N, float v[4][3], uint32_t b = ~0u) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t c = cell_qb(b == ~0u ? blockIdx.x : b, q);
    if (FULL || c < N) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        if constexpr (NT)
          v[q][e] = __builtin_nontemporal_load(p + 3 * c + e);
        else
          v[q][e] = p[3 * c + e];
      }
      if constexpr (SER) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      v[q][0] = v[q][1] = v[q][2] = 0.0f;
    }
  }
}
template <bool FULL, bool NT = true>
__device__ __forceinline__ void store_cells3_stream(float* p, uint32_t N, const float v[4][3], uint32_t b = ~0u) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t c = cell_qb(b == ~0u ? blockIdx.x : b, q);
    if (FULL || c < N) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        if constexpr (NT)
          __builtin_nontemporal_store(v[q][e], p + 3 * c + e);
        else
          p[3 * c + e] = v[q][e];
      }
    }
  }
}
__device__ __forceinline__ float cell_dot3(const float a[3], const float b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// unit partials of dot(x, y) over 3-component cells
__global__ void __launch_bounds__(kBlock) k_dot_partial(const float* __restrict__ x,
                                                        const float* __restrict__ y, uint32_t N, uint32_t U,
                                                        float* partial) {
  __shared__ float lds[16];
  float a[4][3], b[4][3], t[4];
  load_cells3<false>(x, N, a);
  load_cells3<false>(y, N, b);
#pragma unroll
  for (int q = 0; q < 4; ++q) t[q] = cell_dot3(a[q], b[q]);
  quarter_trees(t, lds);
  __syncthreads();
  const uint32_t UB = 4 / U, unit = blockIdx.x * UB + threadIdx.x;
  if (threadIdx.x < UB && (size_t)unit * U * kRedChunkCells < N) partial[unit] = unit_value_q(lds, U, threadIdx.x);
}

// Reference-order group partials (test mode, launch_ref_norm_partials /
// launch_ref_cgs_dots): one wavefront per 64-DOF group, four per block.
__global__ void __launch_bounds__(256) k_ref_norm_partials(const float* __restrict__ v, uint32_t n3,
                                                          float* partial, uint32_t ng) {
  const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  const size_t i = (size_t)g * 64 + l;
  float x = 0.0f;
  if (i < n3) {
    const float a = v[i];
    x = a * a;  // norm_sq_partial: val * val
  }
  x = ref_tree64(x);
  if (l == 0 && g < ng) partial[g] = x;
}
__global__ void __launch_bounds__(256) k_ref_cgs_dots(const float* __restrict__ w, const float* __restrict__ basis,
                                                     const float* __restrict__ binv, size_t stride, uint32_t n3,
                                                     float* partial, uint32_t pstride, uint32_t ng) {
  const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63, ii = blockIdx.y;
  const size_t i = (size_t)g * 64 + l;
  float x = 0.0f;
  if (i < n3) {
    const float vv = binv[ii] * basis[(size_t)ii * stride + i];  // V_ii as the reference's scale stored it
    x = vv * w[i];                                               // calc_dots_cgs: v * w_val
  }
  x = ref_tree64(x);
  if (l == 0 && g < ng) partial[(size_t)ii * pstride + g] = x;
}

// norm outputs of a finished dot: mode 1: out = sqrt(s); mode 2: also inv, g0
__device__ __forceinline__ void norm_out(float s, int mode, float* out, float* inv, float* g0, float* host_out) {
  const float nrm = sqrtf(s);
  out[0] = nrm;
  if (host_out) host_out[0] = nrm;  // mapped pinned host memory: the host's read needs no copy
  if (mode == 2) {
    inv[0] = 1.0f / nrm;  // host-side `1.0 / residual_norm` (coupled_solver_fgmres.rs:1872)
    if (g0) g0[0] = nrm;
  }
}

// g_len > 0 (mode 2): g = [||r||, 0, ..., 0] of length g_len (the zero fill of
// coupled_solver_fgmres.rs:1880-1890 done here instead of a separate fill)
__global__ void __launch_bounds__(kRedFinalThreads) k_reduce_final(RedSrc r, int mode, float* out, float* inv,
                                                                   float* g0, int g_len, float* host_out) {
  __shared__ float la[kRedMaxSegments], lb[65];
  const float s = red_total<float, kRedFinalThreads>(r, 0, la, lb);
  if (g0)
    for (int k = 1 + (int)threadIdx.x; k < g_len; k += kRedFinalThreads) g0[k] = 0.0f;
  if (threadIdx.x == 0) norm_out(s, mode, out, inv, g0, host_out);
}

// calc_dots_cgs (gmres_cgs.wgsl:28-82): partial[ii * np + unit] = <w, V_ii>, ii = 0..j,
// V_ii = binv[ii] * W_ii, in the cell layout of load_cells3; quarter values
// ql[16 ii + 4 q + w] in LDS, units at the end.
template <bool FULL, bool SER, bool NTB = true>
__device__ __forceinline__ void cgs_dots_cells(const float* __restrict__ w, const float* __restrict__ basis,
                                               const float* __restrict__ binv, size_t stride, int j, uint32_t N,
                                               float* ql) {
  float wv[4][3];
  load_cells3<FULL>(w, N, wv);
  for (int ii = 0; ii <= j; ++ii) {
    const float sc = binv[ii];
    float v[4][3], t[4];
    load_cells3<FULL, NTB, SER>(basis + (size_t)ii * stride, N, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 3; ++e) v[q][e] = sc * v[q][e];
      t[q] = cell_dot3(wv[q], v[q]);
    }
    quarter_trees(t, ql + 16 * ii);
  }
}
template <bool SER>
__global__ void __launch_bounds__(kBlock) k_cgs_dots(const float* __restrict__ w,
                                                     const float* __restrict__ basis,
                                                     const float* __restrict__ binv, size_t stride,
                                                     int j, uint32_t N, uint32_t U, float* partial, uint32_t np,
                                                     uint32_t tb) {
  __shared__ float ql[16 * 64];
  // blocks from tb on read the basis with the default policy: their lines stay
  // in the Infinity Cache for the update, which walks the blocks top-down
  if (blockIdx.x < tb) {
    if (block_full(N))
      cgs_dots_cells<true, SER>(w, basis, binv, stride, j, N, ql);
    else
      cgs_dots_cells<false, SER>(w, basis, binv, stride, j, N, ql);
  } else {
    if (block_full(N))
      cgs_dots_cells<true, SER, false>(w, basis, binv, stride, j, N, ql);
    else
      cgs_dots_cells<false, SER, false>(w, basis, binv, stride, j, N, ql);
  }
  __syncthreads();
  const uint32_t UB = 4 / U;
  for (uint32_t idx = threadIdx.x; idx < (uint32_t)(j + 1) * UB; idx += kBlock) {
    const uint32_t ii = idx / UB, u = idx % UB, unit = blockIdx.x * UB + u;
    if ((size_t)unit * U * kRedChunkCells < N) partial[(size_t)ii * np + unit] = unit_value_q(ql + 16 * ii, U, u);
  }
}

// Latency form of the CGS passes for small meshes (round 5): with a few
// blocks on a mostly idle chip each basis vector's loads are a dependent
// round trip of their own when the loop over ii issues one vector at a time,
// so C0's dots / update ran ≈ 10 / 12 us for ≈ 1 us of bytes.  Here KB
// vectors are loaded together before any of them is used, and the dots are
// spread over blockIdx.y (KB vectors per block, w read by each): the same
// cell terms, quarter trees and unit values per vector and chunk, the update's
// corrections accumulated in ii order as before.
#ifndef CFD_CGS_LAT_MAX_CELLS
#define CFD_CGS_LAT_MAX_CELLS (1u << 17)
#endif
constexpr int kCgsLatDots = 4, kCgsLatUpdate = 20;
template <bool FULL, int KB>
__device__ __forceinline__ void cgs_dots_cells_batch(const float* __restrict__ w, const float* __restrict__ basis,
                                                     const float* __restrict__ binv, size_t stride, int ii0, int j,
                                                     uint32_t N, float* ql) {
  float wv[4][3], v[KB][4][3];
  load_cells3<FULL>(w, N, wv);
#pragma unroll
  for (int k = 0; k < KB; ++k) load_cells3<FULL>(basis + (size_t)min(ii0 + k, j) * stride, N, v[k]);
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    if (ii0 + k > j) break;
    const float sc = binv[ii0 + k];
    float t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 3; ++e) v[k][q][e] = sc * v[k][q][e];
      t[q] = cell_dot3(wv[q], v[k][q]);
    }
    quarter_trees(t, ql + 16 * k);
  }
}
__global__ void __launch_bounds__(kBlock) k_cgs_dots_lat(const float* __restrict__ w,
                                                         const float* __restrict__ basis,
                                                         const float* __restrict__ binv, size_t stride, int j,
                                                         uint32_t N, uint32_t U, float* partial, uint32_t np) {
  constexpr int KB = kCgsLatDots;
  __shared__ float ql[16 * KB];
  const int ii0 = (int)blockIdx.y * KB;
  if (block_full(N))
    cgs_dots_cells_batch<true, KB>(w, basis, binv, stride, ii0, j, N, ql);
  else
    cgs_dots_cells_batch<false, KB>(w, basis, binv, stride, ii0, j, N, ql);
  __syncthreads();
  const uint32_t UB = 4 / U, nk = (uint32_t)min(KB, j + 1 - ii0);
  for (uint32_t idx = threadIdx.x; idx < nk * UB; idx += kBlock) {
    const uint32_t k = idx / UB, u = idx % UB, unit = blockIdx.x * UB + u;
    if ((size_t)unit * U * kRedChunkCells < N) partial[(size_t)(ii0 + k) * np + unit] = unit_value_q(ql + 16 * k, U, u);
  }
}

// reduce_dots_cgs (gmres_cgs.wgsl:86-120): H[j][ii] for ii = blockIdx.x
__global__ void __launch_bounds__(kRedFinalThreads) k_cgs_reduce(RedSrc r, int j, float* H, int m1) {
  __shared__ float la[kRedMaxSegments], lb[65];
  const int ii = blockIdx.x;
  const float s = red_total<float, kRedFinalThreads>(r, (uint32_t)ii, la, lb);
  if (threadIdx.x == 0) H[(size_t)j * m1 + ii] = s;
}

// update_w_cgs (gmres_cgs.wgsl:125-166) fused with the ||w||^2 unit partial; the
// updated w is written straight into basis slot j+1 (unnormalised, see binv).
// NTB: nontemporal basis loads and store of the new vector (the default);
// false when the whole basis stays in the caches (small meshes, see
// launch_cgs_update_norm)
template <bool FULL, bool SER, bool NTB>
__device__ __forceinline__ void cgs_update_cells(const float* __restrict__ w, float* basis, size_t stride, int j,
                                                 const float* hcol, const float* scol, uint32_t N, float t[4],
                                                 uint32_t b) {
  float corr[4][3] = {};
  for (int ii = 0; ii <= j; ++ii) {
    const float h = hcol[ii], sc = scol[ii];
    float v[4][3];
    load_cells3<FULL, NTB, SER>(basis + (size_t)ii * stride, N, v, b);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 3; ++e) corr[q][e] += h * (sc * v[q][e]);
  }
  float wn[4][3];
  load_cells3<FULL>(w, N, wn, b);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int e = 0; e < 3; ++e) wn[q][e] = wn[q][e] - corr[q][e];
    t[q] = cell_dot3(wn[q], wn[q]);
  }
  store_cells3_stream<FULL, NTB>(basis + (size_t)(j + 1) * stride, N, wn, b);
}
// k_cgs_reduce's totals computed by every block of the update for itself (one
// GPU, at most 256 padded units: meshes up to ≈ 260 k cells).  The canonical
// total of a vector (red_total: segment trees of GU units, then the tree over
// the P segment values) is the pairwise tree over its unit partials padded
// with +0 to T = P GU values; here L = T / K lanes hold K = min(4, T)
// consecutive units each and a lane tree finishes it -- the same tree.  All
// (j + 1) L lane slots are loaded before any tree (RB rounds of the block in
// flight).  hcol[ii] = the total of vector ii.
template <int NT = kBlock>
__device__ __forceinline__ void cgs_reduce_local(const RedSrc& r, int j, float* hcol) {
  const uint32_t T = pow2_ceil(r.nseg) * r.G, K = T >= 4 ? 4u : T, L = T / K;
  const uint32_t slots = (uint32_t)(j + 1) * L;
  constexpr int RB = NT >= 1024 ? 1 : 4;  // 1,024 threads: one slot each per round (registers)
  for (uint32_t base = 0; base < slots; base += RB * NT) {
    float e[RB][4];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      const uint32_t sl = base + rr * NT + threadIdx.x;
      const uint32_t ii = sl / L, k0 = (sl % L) * K;
      const float* pv = r.p + (size_t)ii * r.stride;
      if (K == 4 && sl < slots && k0 + 3 < r.nchunks) {  // stride and k0 multiples of 4
        const float4 q = *reinterpret_cast<const float4*>(pv + k0);
        e[rr][0] = q.x;
        e[rr][1] = q.y;
        e[rr][2] = q.z;
        e[rr][3] = q.w;
        continue;
      }
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) e[rr][q] = (sl < slots && q < K && k0 + q < r.nchunks) ? pv[k0 + q] : 0.0f;
    }
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      float v = K == 4 ? (e[rr][0] + e[rr][1]) + (e[rr][2] + e[rr][3]) : (K == 2 ? e[rr][0] + e[rr][1] : e[rr][0]);
      for (uint32_t st = 1; st < L; st <<= 1) v = v + __shfl_down(v, st);
      const uint32_t sl = base + rr * NT + threadIdx.x;
      if (sl < slots && sl % L == 0) hcol[sl / L] = v;
    }
  }
}

// FR: the CGS totals reduced in the kernel (cgs_reduce_local from the dots'
// unit partials fr; block 0 stores the Hessenberg column) instead of by
// k_cgs_reduce -- one launch fewer per FGMRES iteration on small meshes
template <bool SER, bool NTB = true, bool FR = false>
__global__ void __launch_bounds__(kBlock) k_cgs_update_norm(const float* __restrict__ w,
                                                            float* basis,
                                                            const float* __restrict__ binv,
                                                            size_t stride, int j,
                                                            float* __restrict__ H, int m1,
                                                            uint32_t N, uint32_t U, float* partial, int rev,
                                                            RedSrc fr) {
  __shared__ float hcol[64], scol[64], ql[16];
  const uint32_t b = rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;  // rev: top-down (after the dots)
  if constexpr (FR) {
    if (threadIdx.x <= (unsigned)j) scol[threadIdx.x] = binv[threadIdx.x];
    cgs_reduce_local(fr, j, hcol);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x <= (unsigned)j) H[(size_t)j * m1 + threadIdx.x] = hcol[threadIdx.x];
  } else {
    if (threadIdx.x <= (unsigned)j) {
      hcol[threadIdx.x] = H[(size_t)j * m1 + threadIdx.x];
      scol[threadIdx.x] = binv[threadIdx.x];
    }
    __syncthreads();
  }
  float t[4];
  if (block_full(N, b))
    cgs_update_cells<true, SER, NTB>(w, basis, stride, j, hcol, scol, N, t, b);
  else
    cgs_update_cells<false, SER, NTB>(w, basis, stride, j, hcol, scol, N, t, b);
  quarter_trees(t, ql);
  __syncthreads();
  const uint32_t UB = 4 / U, unit = b * UB + threadIdx.x;
  if (threadIdx.x < UB && (size_t)unit * U * kRedChunkCells < N) partial[unit] = unit_value_q(ql, U, threadIdx.x);
}

// Latency form of the update (small meshes, see k_cgs_dots_lat): blocks of
// 1,024 threads, one cell per thread -- thread t of block b holds cell
// 1024 b + t, so wavefront t / 64 holds quarter (t / 64) % 4 of chunk t / 256,
// the cells of load_cells3's quarter -- and the first kCgsLatUpdate basis
// vectors (3 floats each) loaded with w before the Hessenberg column is
// known (with FR, while the totals are reduced): one round trip for
// j < kCgsLatUpdate.  Corrections accumulated in ii order, the same norm
// quarter trees and unit values as k_cgs_update_norm.
template <bool FR>
__global__ void __launch_bounds__(1024) k_cgs_update_norm_lat(const float* __restrict__ w, float* basis,
                                                              const float* __restrict__ binv, size_t stride, int j,
                                                              float* __restrict__ H, int m1, uint32_t N, uint32_t U,
                                                              float* partial, RedSrc fr) {
  constexpr int KB = kCgsLatUpdate;
  __shared__ float hcol[64], scol[64], ql[16];
  const uint32_t t = threadIdx.x;
  const size_t c = (size_t)blockIdx.x * 1024u + t;
  const bool in = c < N;
  const size_t cc = in ? c : 0;
  float wn[3], v[KB][3];
#pragma unroll
  for (int e = 0; e < 3; ++e) wn[e] = w[3 * cc + e];
#pragma unroll
  for (int k = 0; k < KB; ++k)
#pragma unroll
    for (int e = 0; e < 3; ++e) v[k][e] = basis[(size_t)min(k, j) * stride + 3 * cc + e];
  if (t <= (unsigned)j) scol[t] = binv[t];
  if constexpr (FR) {
    cgs_reduce_local<1024>(fr, j, hcol);
  } else {
    if (t <= (unsigned)j) hcol[t] = H[(size_t)j * m1 + t];
  }
  __syncthreads();
  if constexpr (FR) {
    if (blockIdx.x == 0 && t <= (unsigned)j) H[(size_t)j * m1 + t] = hcol[t];
  }
  float corr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    if (k <= j) {  // predicated, not a break: v stays in registers
      const float h = hcol[k], sc = scol[k];
#pragma unroll
      for (int e = 0; e < 3; ++e) corr[e] += h * (sc * v[k][e]);
    }
  }
  for (int ii0 = KB; ii0 <= j; ii0 += KB) {  // j >= KB: further batches
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int e = 0; e < 3; ++e) v[k][e] = basis[(size_t)min(ii0 + k, j) * stride + 3 * cc + e];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (ii0 + k <= j) {
        const float h = hcol[ii0 + k], sc = scol[ii0 + k];
#pragma unroll
        for (int e = 0; e < 3; ++e) corr[e] += h * (sc * v[k][e]);
      }
    }
  }
  float tq = 0.0f;  // cells past N: 0 (load_cells3's zero cells)
  if (in) {
#pragma unroll
    for (int e = 0; e < 3; ++e) wn[e] = wn[e] - corr[e];
    tq = cell_dot3(wn, wn);
#pragma unroll
    for (int e = 0; e < 3; ++e) basis[(size_t)(j + 1) * stride + 3 * c + e] = wn[e];
  }
  const float r = wave_tree64(tq);
  if (red_lane() == 0) ql[t >> 6] = r;
  __syncthreads();
  const uint32_t UB = 4 / U, unit = blockIdx.x * UB + t;
  if (t < UB && (size_t)unit * U * kRedChunkCells < N) partial[unit] = unit_value_q(ql, U, t);
}

// reduce_final_and_finish_norm (gmres_ops.wgsl:270-293) + update_hessenberg_givens
// (gmres_logic.wgsl:24-76).
__global__ void __launch_bounds__(kRedFinalThreads) k_norm_givens(RedSrc r, int j, float* H, int m1,
                                                                  float* givens, float* g, float* binv,
                                                                  float* resid_hist, float* host_resid) {
  __shared__ float la[kRedMaxSegments], lb[65];
  // Hessenberg column j and the rotations so far, staged in LDS by the block
  // (issued before the reduction): the serial Givens chain then makes LDS
  // round trips instead of dependent global ones
  float* Hc = H + (size_t)j * m1;
  float hv = 0.0f, gva = 0.0f, gvb = 0.0f;
  const uint32_t t = threadIdx.x;
  if (t <= (uint32_t)j) hv = Hc[t];
  if (t < (uint32_t)j) {
    gva = givens[2 * t];
    gvb = givens[2 * t + 1];
  }
  const float s = red_total<float, kRedFinalThreads>(r, 0, la, lb);  // ends with a barrier
  float* hc = la;         // [j + 2]
  float* gv = la + 128;   // [2 j]
  if (t <= (uint32_t)j) hc[t] = hv;
  if (t < (uint32_t)j) {
    gv[2 * t] = gva;
    gv[2 * t + 1] = gvb;
  }
  __syncthreads();
  if (t != 0) return;
  // norm_givens_out's operations, on the staged values
  const float norm = sqrtf(s);
  hc[j + 1] = norm;
  binv[j + 1] = norm > 1e-20f ? 1.0f / norm : 0.0f;
  for (int ii = 0; ii < j; ++ii) {
    const float hij = hc[ii], hi1j = hc[ii + 1];
    const float cc = gv[2 * ii], ss = gv[2 * ii + 1];
    hc[ii] = cc * hij + ss * hi1j;
    hc[ii + 1] = -ss * hij + cc * hi1j;
  }
  const float hjj = hc[j], hj1j = hc[j + 1];
  float cc = 1.0f, ss = 0.0f;
  const float rho = sqrtf(hjj * hjj + hj1j * hj1j);
  if (fabsf(rho) > 1e-20f) {
    cc = hjj / rho;
    ss = hj1j / rho;
  }
  givens[2 * j] = cc;
  givens[2 * j + 1] = ss;
  hc[j] = rho;
  hc[j + 1] = 0.0f;
  for (int ii = 0; ii <= j + 1; ++ii) Hc[ii] = hc[ii];
  const float gj = g[j], gj1 = g[j + 1];
  g[j] = cc * gj + ss * gj1;
  const float gn = -ss * gj + cc * gj1;
  g[j + 1] = gn;
  resid_hist[j] = fabsf(gn);
  // the host's lag-model read (coupled_solver.rs:326-435): written straight into
  // pinned host memory, so no copy is enqueued per iteration
  if (host_resid) host_resid[0] = fabsf(gn);
}

// solve_triangular (gmres_logic.wgsl:78-104), single lane
// H's first k columns and g are staged in LDS by the whole block, then one
// lane runs the reference's back substitution from LDS (the same operations
// in the same order; every H / y access was a dependent global round trip)
__global__ void __launch_bounds__(256) k_solve_triangular(const float* H, const float* g, float* y, int k, int m1) {
  __shared__ float hs[64 * 64], gs[64], ys[64];
  for (int e = threadIdx.x; e < k * m1; e += blockDim.x) hs[e] = H[e];
  if (threadIdx.x < (unsigned)k) gs[threadIdx.x] = g[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int li = 0; li < k; ++li) {
      const int i = k - 1 - li;
      float sum = gs[i];
      // unrolled: the LDS loads of 8 terms issue together, only the
      // subtractions form the chain (same operations, same order)
#pragma unroll 8
      for (int jj = i + 1; jj < k; ++jj) sum -= hs[jj * m1 + i] * ys[jj];
      const float diag = hs[i * m1 + i];
      ys[i] = (fabsf(diag) > 1e-12f) ? sum / diag : 0.0f;
    }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)k) y[threadIdx.x] = ys[threadIdx.x];
}

// the preconditioned vectors Z_i are read once per restart cycle here (nontemporal)
__device__ __forceinline__ float4 ld4_upd(const float* p) { return ldv<true, float4>(p); }
template <bool SER>
__device__ __forceinline__ void upd_wait() {
  if constexpr (SER) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// basis_size x axpy_from_y (gmres_ops.wgsl:96-105) fused: x = y_i * z_i + x, i ascending
// SER: one Z load in flight per thread, on meshes of at least
// CFD_CGS_SER_MIN_CELLS cells (A/B C2: 614 -> 583 us)
template <bool SER>
__global__ void __launch_bounds__(kBlock) k_update_x(float* x, const float* __restrict__ z,
                                                     size_t stride, const float* __restrict__ y,
                                                     int k, size_t n) {
  const size_t e = 4 * ((size_t)blockIdx.x * kBlock + threadIdx.x);
  if (e >= n) return;
  if (e + 3 < n) {  // 4 elements per thread, 16-byte loads (slots are 256-byte aligned)
    float4 xv = *reinterpret_cast<const float4*>(x + e);
    int ii = 0;
    for (; ii + 1 < k; ii += 2) {
      const float4 z0 = ld4_upd(z + (size_t)ii * stride + e);
      upd_wait<SER>();
      const float4 z1 = ld4_upd(z + (size_t)(ii + 1) * stride + e);
      upd_wait<SER>();
      const float y0 = y[ii], y1 = y[ii + 1];
      xv.x = y0 * z0.x + xv.x;
      xv.y = y0 * z0.y + xv.y;
      xv.z = y0 * z0.z + xv.z;
      xv.w = y0 * z0.w + xv.w;
      xv.x = y1 * z1.x + xv.x;
      xv.y = y1 * z1.y + xv.y;
      xv.z = y1 * z1.z + xv.z;
      xv.w = y1 * z1.w + xv.w;
    }
    if (ii < k) {
      const float4 z0 = ld4_upd(z + (size_t)ii * stride + e);
      const float y0 = y[ii];
      xv.x = y0 * z0.x + xv.x;
      xv.y = y0 * z0.y + xv.y;
      xv.z = y0 * z0.z + xv.z;
      xv.w = y0 * z0.w + xv.w;
    }
    *reinterpret_cast<float4*>(x + e) = xv;
    return;
  }
  for (size_t f = e; f < n; ++f) {
    float xv = x[f];
    for (int ii = 0; ii < k; ++ii) xv = y[ii] * z[(size_t)ii * stride + f] + xv;
    x[f] = xv;
  }
}

// Latency form (small meshes, as the CGS passes': k_cgs_dots_lat): 16 of the
// Z vectors' loads issued per round trip instead of 2, the updates applied in
// ascending i as above -- same operations.
__global__ void __launch_bounds__(kBlock) k_update_x_lat(float* x, const float* __restrict__ z, size_t stride,
                                                         const float* __restrict__ y, int k, size_t n) {
  constexpr int KB = 16;
  const size_t e = 4 * ((size_t)blockIdx.x * kBlock + threadIdx.x);
  if (e >= n) return;
  if (e + 3 < n) {
    float4 xv = *reinterpret_cast<const float4*>(x + e);
    for (int ii0 = 0; ii0 < k; ii0 += KB) {
      float4 zb[KB];
#pragma unroll
      for (int q = 0; q < KB; ++q) zb[q] = *reinterpret_cast<const float4*>(z + (size_t)min(ii0 + q, k - 1) * stride + e);
#pragma unroll
      for (int q = 0; q < KB; ++q) {
        if (ii0 + q < k) {
          const float yq = y[ii0 + q];
          xv.x = yq * zb[q].x + xv.x;
          xv.y = yq * zb[q].y + xv.y;
          xv.z = yq * zb[q].z + xv.z;
          xv.w = yq * zb[q].w + xv.w;
        }
      }
    }
    *reinterpret_cast<float4*>(x + e) = xv;
    return;
  }
  for (size_t f = e; f < n; ++f) {
    float xv = x[f];
    for (int ii = 0; ii < k; ++ii) xv = y[ii] * z[(size_t)ii * stride + f] + xv;
    x[f] = xv;
  }
}

}  // namespace

void launch_dot_partial(const float* x, const float* y, uint32_t N, uint32_t U, float* partial, hipStream_t s) {
  if (N) hipLaunchKernelGGL(k_dot_partial, dim3(red_blocks(N)), dim3(kBlock), 0, s, x, y, N, U, partial);
}
void launch_ref_norm_partials(const float* v, uint32_t n3, float* partial, hipStream_t s) {
  const uint32_t ng = (n3 + 63) / 64;
  if (ng) hipLaunchKernelGGL(k_ref_norm_partials, dim3((ng + 3) / 4), dim3(256), 0, s, v, n3, partial, ng);
}
void launch_ref_cgs_dots(const float* w, const float* basis, const float* binv, size_t stride, int j, uint32_t n3,
                         float* partial, uint32_t pstride, hipStream_t s) {
  const uint32_t ng = (n3 + 63) / 64;
  if (ng)
    hipLaunchKernelGGL(k_ref_cgs_dots, dim3((ng + 3) / 4, (unsigned)(j + 1)), dim3(256), 0, s, w, basis, binv, stride,
                       n3, partial, pstride, ng);
}
void launch_reduce_final(const RedSrc& r, int mode, float* out, float* inv, float* g0, int g_len, float* host_out,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(kRedFinalThreads), 0, s, r, mode, out, inv, g0, g_len,
                     host_out);
}
bool cgs_latency_form(uint32_t N) { return N <= CFD_CGS_LAT_MAX_CELLS; }
bool cgs_serial_form(uint32_t N) { return N >= CFD_CGS_SER_MIN_CELLS; }
void launch_cgs_dots(const float* w, const float* basis, const float* binv, size_t stride, int j, uint32_t N,
                     uint32_t U, float* partial, uint32_t np, hipStream_t s, size_t keep_bytes, bool lat) {
  if (!N) return;
  const uint32_t nb = red_blocks(N);
  if (lat) {
    if (!cgs_latency_form(N)) throw std::logic_error("launch_cgs_dots: latency form past its size limit");
    hipLaunchKernelGGL(k_cgs_dots_lat, dim3(nb, (unsigned)(j + kCgsLatDots) / kCgsLatDots), dim3(kBlock), 0, s, w,
                       basis, binv, stride, j, N, U, partial, np);
    return;
  }
  // the last blocks whose basis lines (j + 1 vectors + w, 12 B per cell each) fit keep_bytes
  const size_t keep_blocks = keep_bytes / ((size_t)(j + 2) * 12u * 1024u);
  const uint32_t tb = keep_blocks >= nb ? 0u : nb - (uint32_t)keep_blocks;
  if (N >= CFD_CGS_SER_MIN_CELLS)
    hipLaunchKernelGGL(k_cgs_dots<true>, dim3(nb), dim3(kBlock), 0, s, w, basis, binv, stride, j, N, U,
                       partial, np, tb);
  else
    hipLaunchKernelGGL(k_cgs_dots<false>, dim3(nb), dim3(kBlock), 0, s, w, basis, binv, stride, j, N, U,
                       partial, np, tb);
}
void launch_cgs_reduce(const RedSrc& r, int j, float* H, int m1, hipStream_t s) {
  hipLaunchKernelGGL(k_cgs_reduce, dim3(j + 1), dim3(kRedFinalThreads), 0, s, r, j, H, m1);
}
bool cgs_reduce_fusable(const RedSrc& r) {
  return !r.seg_src && (uint64_t)pow2_ceil(r.nseg) * r.G <= 256u;
}
void launch_cgs_update_norm(const float* w, float* basis, const float* binv, size_t stride, int j, float* H,
                            int m1, uint32_t N, uint32_t U, float* partial, hipStream_t s, bool rev, bool ntb,
                            const RedSrc* fr, bool lat) {
  if (!N) return;
  const bool ser = N >= CFD_CGS_SER_MIN_CELLS;
  if (fr && (ser || !cgs_reduce_fusable(*fr)))
    throw std::logic_error("launch_cgs_update_norm: fused CGS reduction past its size limit");
  if (lat && !cgs_latency_form(N)) throw std::logic_error("launch_cgs_update_norm: latency form past its size limit");
  if (lat) {  // default-policy loads and store (ntb and rev do not apply)
    hipLaunchKernelGGL(fr ? k_cgs_update_norm_lat<true> : k_cgs_update_norm_lat<false>, dim3((N + 1023) / 1024),
                       dim3(1024), 0, s, w, basis, binv, stride, j, H, m1, N, U, partial, fr ? *fr : RedSrc{});
    return;
  }
  auto fn = fr  ? (ntb ? k_cgs_update_norm<false, true, true> : k_cgs_update_norm<false, false, true>)
          : ser ? (ntb ? k_cgs_update_norm<true, true> : k_cgs_update_norm<true, false>)
                : (ntb ? k_cgs_update_norm<false, true> : k_cgs_update_norm<false, false>);
  hipLaunchKernelGGL(fn, dim3(red_blocks(N)), dim3(kBlock), 0, s, w, basis, binv, stride, j, H, m1, N, U, partial,
                     rev ? 1 : 0, fr ? *fr : RedSrc{});
}
void launch_norm_givens(const RedSrc& r, int j, float* H, int m1, float* givens, float* g, float* binv,
                        float* resid_hist, float* host_resid, hipStream_t s) {
  hipLaunchKernelGGL(k_norm_givens, dim3(1), dim3(kRedFinalThreads), 0, s, r, j, H, m1, givens, g, binv,
                     resid_hist, host_resid);
}
void launch_solve_triangular(const float* H, const float* g, float* y, int k, int m1, hipStream_t s) {
  if (k > 64 || m1 > 64) throw std::invalid_argument("solve_triangular: basis larger than 64");
  hipLaunchKernelGGL(k_solve_triangular, dim3(1), dim3(256), 0, s, H, g, y, k, m1);
}
void launch_update_x(float* x, const float* z, size_t stride, const float* y, int k, size_t n,
                     hipStream_t s, bool lat) {
  if (!n) return;
  if (lat && n / 3 <= CFD_CGS_LAT_MAX_CELLS && k > 2) {
    hipLaunchKernelGGL(k_update_x_lat, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, s, x, z, stride, y, k, n);
    return;
  }
  if (n / 3 >= CFD_CGS_SER_MIN_CELLS)
    hipLaunchKernelGGL(k_update_x<true>, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, s, x, z, stride, y, k, n);
  else
    hipLaunchKernelGGL(k_update_x<false>, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, s, x, z, stride, y, k, n);
}

}  // namespace cfd2
