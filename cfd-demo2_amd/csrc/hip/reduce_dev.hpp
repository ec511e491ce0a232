// The canonical reduction order (kernels.hpp: leaf / chunk / segment / total)
// on the device: the trees every reducing kernel shares.
#pragma once
#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

#ifndef CFD_RED_SEGS
#define CFD_RED_SEGS 4  // independent partial loads per lane in the finishing kernels
#endif

// Pairwise tree over the first `active` lanes of the wavefront (a power of
// two <= 64); lane 0 holds the root.  Lane l adds lane l + s at strides
// s = 1, 2, ...: at every level each surviving node is (left + right).
template <class T>
__device__ __forceinline__ T wave_tree(T v, uint32_t active = 64) {
  for (uint32_t st = 1; st < active; st <<= 1) v = v + __shfl_down(v, st);
  return v;
}
// chunk of this wavefront in a reduction kernel (4 chunks per 256-thread block)
__device__ __forceinline__ uint32_t red_chunk() { return blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); }
__device__ __forceinline__ uint32_t red_lane() { return threadIdx.x & 63; }

// Segment values of U consecutive-in-steps segments s0, s0 + sstep, ... from
// chunk partials pv[k] (k < nchunks, missing chunks +0): lane l holds chunk
// slots [l K, l K + K) of the segment, K = min(4, G / 64) ... (G <= 256).
template <class T, int U>
__device__ __forceinline__ void seg_trees(const T* __restrict__ pv, uint32_t nchunks, uint32_t G, uint32_t s0,
                                          uint32_t sstep, uint32_t nseg, T out[U]) {
  const uint32_t lane = red_lane();
  const uint32_t K = G >= 256 ? 4u : (G >= 128 ? 2u : 1u);
  const uint32_t L = G / K;  // active lanes (power of two)
  T e[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t sg = s0 + u * sstep;
    const uint64_t k0 = (uint64_t)sg * G + (uint64_t)lane * K;
    if constexpr (sizeof(T) == 4) {
      // 4 chunk slots in one 16-byte load (per-vector strides are multiples of 4)
      if (K == 4 && sg < nseg && k0 + 3 < nchunks) {
        const float4 q = *reinterpret_cast<const float4*>(pv + k0);
        e[u][0] = q.x;
        e[u][1] = q.y;
        e[u][2] = q.z;
        e[u][3] = q.w;
        continue;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t k = k0 + q;
      e[u][q] = (sg < nseg && lane < L && (uint32_t)q < K && k < nchunks) ? pv[k] : T(0);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    T v;
    if (K == 4)
      v = (e[u][0] + e[u][1]) + (e[u][2] + e[u][3]);
    else if (K == 2)
      v = e[u][0] + e[u][1];
    else
      v = e[u][0];
    out[u] = wave_tree(v, L);
  }
}

__host__ __device__ __forceinline__ uint32_t pow2_ceil(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// Segment values of one vector's unit partials pv[0, nunits) into LDS a[0, P)
// (P = pow2 >= nseg; segments past nseg are +0): segment sg = pairwise tree over
// its GU unit values pv[sg GU ..] (missing units +0).  A group of LS = GU / K
// lanes serves one segment, each lane K = min(4, GU) consecutive units (one
// 16-byte load when K = 4), then the tree over the group's lanes.  A wavefront
// iterates as a whole, so every shuffle reads a live lane.
template <class T, int NT>
__device__ __forceinline__ void seg_values(const T* __restrict__ pv, uint32_t nunits, uint32_t GU, uint32_t nseg,
                                           uint32_t P, T* a) {
  const uint32_t K = GU >= 4 ? 4u : GU;
  const uint32_t LS = GU / K;
  const uint32_t slots = P * LS;  // a multiple of 64 when >= 64
  constexpr int R = CFD_RED_SEGS;  // independent loads in flight per lane
  for (uint32_t base = threadIdx.x & ~63u; base < slots; base += R * NT) {
    T e[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t t = base + r * NT + red_lane();
      const uint32_t sg = t / LS;
      const uint64_t k0 = (uint64_t)sg * GU + (uint64_t)(t % LS) * K;
      if constexpr (sizeof(T) == 4) {
        if (K == 4 && sg < nseg && k0 + 3 < nunits) {
          const float4 q = *reinterpret_cast<const float4*>(pv + k0);
          e[r][0] = q.x;
          e[r][1] = q.y;
          e[r][2] = q.z;
          e[r][3] = q.w;
          continue;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        e[r][q] = (sg < nseg && (uint32_t)q < K && k0 + q < nunits) ? pv[k0 + q] : T(0);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      T v = K == 4 ? (e[r][0] + e[r][1]) + (e[r][2] + e[r][3]) : (K == 2 ? e[r][0] + e[r][1] : e[r][0]);
      for (uint32_t st = 1; st < LS; st <<= 1) v = v + __shfl_down(v, st);
      const uint32_t t = base + r * NT + red_lane();
      if (t < slots && t % LS == 0) a[t / LS] = v;
    }
  }
}

// Pairwise tree over a[0, P) (P a power of two <= kRedMaxSegments): blocks of
// 64 by wavefront trees, then the <= 64 block values by one wavefront -- the
// same bits as halving level by level.  b needs 65 entries.  Every thread
// returns the total.
template <class T, int NT>
__device__ __forceinline__ T total_tree(const T* a, uint32_t P, T* b) {
  constexpr uint32_t NW = NT / 64;
  const uint32_t w = threadIdx.x >> 6, lane = red_lane();
  __syncthreads();  // a[] complete
  uint32_t Q = P;
  const T* src = a;
  if (P > 64) {
    for (uint32_t gi = w; gi < P / 64; gi += NW) {
      const T v = wave_tree(a[64 * gi + lane], 64);
      if (lane == 0) b[gi] = v;
    }
    __syncthreads();
    Q = P / 64;
    src = b;
  }
  if (w == 0) {
    const T v = wave_tree(lane < Q ? src[lane] : T(0), Q);
    if (lane == 0) b[64] = v;
  }
  __syncthreads();
  const T tot = b[64];
  __syncthreads();  // the caller may reuse the LDS
  return tot;
}

// The 64-wide halving tree of the reference's workgroup reductions (stride
// 32 .. 1: lane l adds lane l + stride, gmres_ops.wgsl:177-182) as one
// wavefront's shuffles -- the same pairs, lane 0 holds the result.
template <class T>
__device__ __forceinline__ T ref_tree64(T v) {
  for (int st = 32; st > 0; st >>= 1) v = v + __shfl_down(v, st);
  return v;
}

// Reference reduction order (RedSrcT::order, test mode): the total of vector v
// from the reference's 64-DOF group partials.  Every thread returns it.
template <class T, int NT>
__device__ __forceinline__ T ref_total(const RedSrcT<T>& r, uint32_t v, T* b) {
  const T* p = r.p + (size_t)v * r.stride;
  __syncthreads();
  if (r.order == 1) {  // reduce_final: one thread, the partials in order
    if (threadIdx.x == 0) {
      T s = T(0);
      for (uint32_t k = 0; k < r.nchunks; ++k) s += p[k];
      b[64] = s;
    }
  } else if (threadIdx.x < 64) {  // reduce_dots_cgs: strided lane sums, then the tree
    T s = T(0);
    for (uint32_t k = threadIdx.x; k < r.nchunks; k += 64) s += p[k];
    s = ref_tree64(s);
    if (threadIdx.x == 0) b[64] = s;
  }
  __syncthreads();
  const T tot = b[64];
  __syncthreads();  // the caller may reuse the LDS
  return tot;
}

// Total of vector v of reduction r by the whole block (NT threads): the
// segment values into LDS a[0, P) (+0 padding to P = pow2 >= nseg), then the
// pairwise tree over them.  Every thread returns the total.
template <class T, int NT>
__device__ __forceinline__ T red_total(const RedSrcT<T>& r, uint32_t v, T* a, T* b) {
  if (r.order) return ref_total<T, NT>(r, v, b);
  const uint32_t P = pow2_ceil(r.nseg);
  if (r.seg_src) {  // distributed: gathered segment values
    const size_t blk = (size_t)r.nvec * r.stride;
    for (uint32_t sg = threadIdx.x; sg < P; sg += NT) {
      T val = T(0);
      if (sg < r.nseg) {
        const uint32_t src = r.seg_src[sg];
        val = r.p[(size_t)(src >> 20) * blk + (size_t)v * r.stride + (src & 0xFFFFFu)];
      }
      a[sg] = val;
    }
  } else {  // one GPU: segment trees of the unit partials
    seg_values<T, NT>(r.p + (size_t)v * r.stride, r.nchunks, r.G, r.nseg, P, a);
  }
  return total_tree<T, NT>(a, P, b);
}
#ifndef CFD_RED_FINAL_THREADS
#define CFD_RED_FINAL_THREADS 1024
#endif
constexpr int kRedFinalThreads = CFD_RED_FINAL_THREADS;

// wave_tree(v, 64) without LDS traffic: strides 1..8 by DPP row shifts (lane
// l adds lane l + s of its row of 16; only lanes whose chain stays inside the
// row are read), strides 16 and 32 from the row roots by lane reads -- the
// same additions in the same order.  Valid in every lane.
template <int S>
__device__ __forceinline__ float row_down(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + S, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_tree64(float v) {
  v = v + row_down<1>(v);
  v = v + row_down<2>(v);
  v = v + row_down<4>(v);
  v = v + row_down<8>(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}
// quarters of the block's chunks: lds[4 q + w] = wave_tree of wavefront w's
// cell terms t[q] (written by lane 0)
__device__ __forceinline__ void quarter_trees(const float t[4], float* lds) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float r = wave_tree64(t[q]);
    if (red_lane() == 0) lds[4 * q + (threadIdx.x >> 6)] = r;
  }
}
// chunk q's value from its 4 quarter values (pairwise)
__device__ __forceinline__ float quarter_chunk(const float* l, int q) {
  return (l[4 * q] + l[4 * q + 1]) + (l[4 * q + 2] + l[4 * q + 3]);
}
// Units of the block's 4 chunk values l[0..3] (kernels.hpp): unit u of U chunks
// = the pairwise tree over them
template <class T>
__device__ __forceinline__ T unit_value(const T* l, uint32_t U, uint32_t u) {
  if (U == 4) return (l[0] + l[1]) + (l[2] + l[3]);
  if (U == 2) return l[2 * u] + l[2 * u + 1];
  return l[u];
}
// ... from the 16 quarter values ql[4 q + w] of the block's chunks
__device__ __forceinline__ float unit_value_q(const float* ql, uint32_t U, uint32_t u) {
  float l[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) l[q] = quarter_chunk(ql, q);
  return unit_value(l, U, u);
}
// The block's unit partials of one sum from its quarter values l[chunk q][quarter
// w] (after the barrier): thread u < 4 / U forms unit u -- the chunks' quarters
// pairwise, then unit_value -- and stores it to dst[unit] if the unit starts
// inside the mesh.  A kernel with several sums picks the thread of each (sum, u).
__device__ __forceinline__ void unit_partials(const double (*l)[4], uint32_t U, uint32_t np, uint32_t N, uint32_t lb,
                                              double* dst, uint32_t u = threadIdx.x) {
  const uint32_t UB = 4 / U;
  if (u >= UB) return;
  const uint32_t unit = lb * UB + u;
  double ch[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) ch[q] = (l[q][0] + l[q][1]) + (l[q][2] + l[q][3]);
  const double v = unit_value(ch, U, u);
  if ((uint64_t)unit * U * kRedChunkCells < N && unit < np) dst[unit] = v;
}
// ---- the block skeleton of every kernel with f64 cell sums ----
// Block lb of such a kernel takes kRedBlockCells cells (kernels.hpp): chunk q is
// its 256 cells of round q, wavefront w the chunk's quarter w.  A kernel keeps
// `__shared__ double lsum[NS][4][4]` ([sum][chunk q][quarter w]), calls
// sum_accumulate with its per-cell term, folds its maxima (if any) into LDS of
// its own, and after one __syncthreads() calls sum_store: every sum it writes
// has the bits of the canonical tree.
//
// The accumulate half (no barrier): per round, t[0, NS) from +0, term(i, t) for
// a cell inside the mesh, then the quarter's shuffle tree of each sum.  Only
// the first LIVE sums are reduced; the others are +0 whatever term left in them.
template <int NS, int LIVE = NS, class Term>
__device__ __forceinline__ void sum_accumulate(double (*lsum)[4][4], uint32_t N, uint32_t lb, Term term) {
  const uint32_t w = threadIdx.x >> 6, lane = red_lane();
  for (uint32_t q = 0; q < 4; ++q) {
    const uint64_t ci = (uint64_t)lb * kRedBlockCells + q * kRedChunkCells + threadIdx.x;
    double t[NS];
#pragma unroll
    for (int f = 0; f < NS; ++f) t[f] = 0.0;
    if (ci < N) term((uint32_t)ci, t);
#pragma unroll
    for (int f = 0; f < LIVE; ++f) {
      const double r = wave_tree(t[f]);
      if (lane == 0) lsum[f][q][w] = r;
    }
    if constexpr (LIVE < NS) {
      if (lane == 0) {
#pragma unroll
        for (int f = LIVE; f < NS; ++f) lsum[f][q][w] = 0.0;
      }
    }
  }
}
// The store half (after the barrier): thread f UB + u, UB = 4 / U units per
// block, stores unit u of sum f to o.partial[f * np + unit] (unit_partials).
template <int NS>
__device__ __forceinline__ void sum_store(const double (*lsum)[4][4], const SumOut& o, uint32_t N, uint32_t lb) {
  const uint32_t UB = 4 / o.U, f = threadIdx.x / UB;
  if (f < NS) unit_partials(lsum[f], o.U, o.np, N, lb, o.partial + (size_t)f * o.np, threadIdx.x % UB);
}
// the block's chunks are all inside the mesh
__device__ __forceinline__ bool block_full(uint32_t N, uint32_t b = ~0u) {
  return (size_t)((b == ~0u ? blockIdx.x : b) + 1) * kRedBlockCells <= N;
}

// ---- maxima and minima as unsigned integers ----
// Non-negative floats order as their bit patterns, every non-NaN float as its
// scalar_value_key; an integer maximum is exact in any order, so none of the
// trees below is part of a result's definition.
// |v| as such a pattern; a NaN counts as +inf, so it is never the smaller one
constexpr uint32_t kDeltaNaN = 0x7f800000u;
__device__ __forceinline__ uint32_t abs_bits(float v) {
  const float d = fabsf(v);
  return d == d ? __float_as_uint(d) : kDeltaNaN;
}
template <bool MIN, class T>
__device__ __forceinline__ T ext(T a, T b) {
  return (MIN ? b < a : b > a) ? b : a;
}
// over the wavefront (the xor butterfly: every lane holds the result)
template <bool MIN, class T>
__device__ __forceinline__ T wave_ext(T v) {
  for (int o = 32; o >= 1; o >>= 1) v = ext<MIN>(v, (T)__shfl_xor(v, o));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) { return wave_ext<false>(v); }
template <class T>
__device__ __forceinline__ T wave_min(T v) { return wave_ext<true>(v); }
// over a 256-thread block, from its four wavefronts' values in LDS (after the barrier)
static_assert(kBlock == 4 * 64, "block_of4_*: four wavefronts per block");
template <bool MIN, class T>
__device__ __forceinline__ T block_of4_ext(const T* l) {
  return ext<MIN>(ext<MIN>(l[0], l[1]), ext<MIN>(l[2], l[3]));
}
template <class T>
__device__ __forceinline__ T block_of4_max(const T* l) { return block_of4_ext<false>(l); }
template <class T>
__device__ __forceinline__ T block_of4_min(const T* l) { return block_of4_ext<true>(l); }

// One block folds per-block values: out[j] = the minimum (j < nmin) or maximum
// over the blocks b < nb of v[nv b + j], j < nv (no block: the neutral element).
template <class T>
__global__ void __launch_bounds__(kBlock) k_block_fold(const T* __restrict__ v, uint32_t nb, uint32_t nv, uint32_t nmin,
                                                       T* out) {
  __shared__ T l[kBlock / 64];
  for (uint32_t j = 0; j < nv; ++j) {
    const bool mn = j < nmin;
    T m = mn ? ~T(0) : T(0);
    for (uint32_t b = threadIdx.x; b < nb; b += kBlock) {
      const T x = v[(size_t)nv * b + j];
      m = mn ? ext<true>(m, x) : ext<false>(m, x);
    }
    m = mn ? wave_min(m) : wave_max(m);
    if (red_lane() == 0) l[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[j] = mn ? block_of4_min(l) : block_of4_max(l);
    __syncthreads();
  }
}

}  // namespace cfd2
