// AMG V-cycle on the big levels: smooth, residual, restrict, prolong and the
// fused level-pair kernels.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "amg_rows.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// smooth_op (amg.wgsl:24-50) restated out-of-place: x_out = mix(x, (b - sigma)/diag, 0.8).
// PRO (post-smoother of a single-GPU / replicated level): the prolongation
// from the coarse level xc that precedes it (k_amg_prolong) is applied to
// every x value as it is read, so x' = x + P xc is never stored -- the same
// f32 operations per value, one launch and one pass over x / agg fewer.
// smooth4: the 4 rows i0..i0+3
// The row operands (b, x, diagonal) are loaded after the slot loop (loading
// them with the row lengths was inside the noise, round 3); in the fused
// post-smoother the row's own prolongation term (agg -> x_c) comes after the
// slots as well (before them: +0.1 ... +0.5 us on every C1 level).
template <bool D16, int MODE, bool PRO = false, bool NT = false>
__device__ __forceinline__ float4 smooth4(const AmgLevelDev& L, const float* __restrict__ x,
                                          const float* __restrict__ b, uint32_t i0,
                                          const float* __restrict__ xc = nullptr) {
  const uchar4 ln = ldv<NT, uchar4>(L.len + i0);
  const uint32_t maxlen = max(max(ln.x, ln.y), max(ln.z, ln.w));
  float sg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  auto step = [&](uint32_t r0, uint32_t rmax) {
    float4 v[kU];
    float xg[kU][4];
    gather_group<D16, MODE, true, PRO, NT>(L, x, i0, r0, rmax, ln, v, xg, xc);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (r0 + u < u4(ln, k)) sg[k] += f4(v[u], k) * xg[u][k];
  };
  if constexpr (MODE != 0) {
    // first slot group peeled: its loads (clamped to the ELL width) do not wait for the lengths
    step(0, (uint32_t)max(L.w, 1) - 1u);
    for (uint32_t r0 = kU; r0 < maxlen; r0 += kU) step(r0, maxlen - 1u);
  } else {
    for (uint32_t r0 = 0; r0 < maxlen; r0 += kU) step(r0, maxlen - 1u);
  }
  const float4 bb = ldv<NT, float4>(b + i0);
  float4 xx = *reinterpret_cast<const float4*>(x + i0);
  const float4 dd = ldv<NT, float4>(L.de + i0);
  if constexpr (PRO) {  // the row's own value, as k_amg_prolong (padding rows get + 0)
    float pc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int4 ag = *reinterpret_cast<const int4*>(L.agg + i0);
    pc[0] += 1.0f * xc[ag.x];
    if (i0 + 1 < L.n) pc[1] += 1.0f * xc[ag.y];
    if (i0 + 2 < L.n) pc[2] += 1.0f * xc[ag.z];
    if (i0 + 3 < L.n) pc[3] += 1.0f * xc[ag.w];
    xx.x += pc[0];
    xx.y += pc[1];
    xx.z += pc[2];
    xx.w += pc[3];
  }
  float4 o;
  o.x = wmix(xx.x, (bb.x - sg[0]) / dd.x, 0.8f);
  o.y = wmix(xx.y, (bb.y - sg[1]) / dd.y, 0.8f);
  o.z = wmix(xx.z, (bb.z - sg[2]) / dd.z, 0.8f);
  o.w = wmix(xx.w, (bb.w - sg[3]) / dd.w, 0.8f);
  return o;
}
// The level's fields the sweep needs first (row lengths, slot values and
// columns, the row ranges, ELL stride and width) and x, b lead the argument
// list: those 16 dwords arrive preloaded in SGPRs (kernarg preload, §4), so
// the first loads wait for no kernarg round trip; the rest of the level
// image comes with L.
template <bool D16, int MODE, bool PRO = false, bool NT = false>
__global__ void __launch_bounds__(kBlock) k_amg_smooth(const uint8_t* len, const float* val, const void* col,
                                                       uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3,
                                                       uint32_t stride, int w, const float* __restrict__ x,
                                                       const float* __restrict__ b, float* __restrict__ x_out,
                                                       AmgLevelDev L, const float* __restrict__ xc) {
  uint32_t i0;
  if (!row_range<kRevSmooth>(r0, r1, r2, r3, i0)) return;
  AmgLevelDev Lk = L;
  Lk.len = len;
  Lk.val = val;
  if constexpr (D16)
    Lk.col16 = static_cast<const int16_t*>(col);
  else
    Lk.col32 = static_cast<const int32_t*>(col);
  Lk.r0 = r0;
  Lk.r1 = r1;
  Lk.r2 = r2;
  Lk.r3 = r3;
  Lk.stride = stride;
  Lk.w = w;
  *reinterpret_cast<float4*>(x_out + i0) = smooth4<D16, MODE, PRO, NT>(Lk, x, b, i0, xc);
}
// The reference's IN-PLACE smooth_op (amg.wgsl:24-50) under one legal
// schedule (test mode, Solver::ref_inplace; oracle kSemInplaceSmoother): the
// 64-row workgroups one after another, every row of a workgroup reading x
// before any of them writes -- so rows of earlier workgroups are read new.
// One block walks the row blocks in order; its 16 threads take 4 rows each
// (smooth4: the same operations as k_amg_smooth).
template <bool D16, int MODE>
__global__ void __launch_bounds__(16) k_amg_smooth_ordered(AmgLevelDev L, float* x, const float* __restrict__ b) {
  for (uint32_t b0 = 0; b0 < L.n; b0 += 64) {
    const uint32_t i0 = b0 + 4 * threadIdx.x;
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i0 < L.n) o = smooth4<D16, MODE>(L, x, b, i0);
    __syncthreads();  // the workgroup's reads complete
    if (i0 < L.n) *reinterpret_cast<float4*>(x + i0) = o;
    __syncthreads();  // visible to the next workgroup's reads
  }
}

// the leading arguments of k_amg_smooth from a level image
#define CFD_AMG_HEAD(L) \
  (L).len, (L).val, ((L).use16 ? (const void*)(L).col16 : (const void*)(L).col32), (L).r0, (L).r1, (L).r2, (L).r3, \
      (L).stride, (L).w

// smooth_op on a level whose x is identically +0 (every coarse level's
// pre-smoother: restrict just cleared it): sigma = +0, so the sweep is the
// elementwise x_out = mix(+0, (b - 0)/diag, 0.8) -- the same f32 operations
// as k_amg_smooth without reading the matrix.
__global__ void __launch_bounds__(kBlock) k_amg_smooth_zero(AmgLevelDev L, const float* __restrict__ b,
                                                            float* __restrict__ x_out) {
  const uint32_t i0 = 4 * row_id();
  if (i0 >= L.n) return;
  const float4 bb = *reinterpret_cast<const float4*>(b + i0);
  const float4 dd = *reinterpret_cast<const float4*>(L.de + i0);
  float4 o;
  o.x = wmix(0.0f, (bb.x - 0.0f) / dd.x, 0.8f);
  o.y = wmix(0.0f, (bb.y - 0.0f) / dd.y, 0.8f);
  o.z = wmix(0.0f, (bb.z - 0.0f) / dd.z, 0.8f);
  o.w = wmix(0.0f, (bb.w - 0.0f) / dd.w, 0.8f);
  *reinterpret_cast<float4*>(x_out + i0) = o;
}

// residual part of restrict_residual (amg.wgsl:80-111): r = b - A x over the full
// row in column order, the diagonal inserted at its rank.
template <bool D16, int MODE, bool NT = false>
__device__ __forceinline__ float4 residual4(const AmgLevelDev& L, const float* __restrict__ x,
                                            const float* __restrict__ b, uint32_t i0) {
  const uchar4 ln = ldv<NT, uchar4>(L.len + i0);
  const uchar4 dr = ldv<NT, uchar4>(L.drank + i0);
  const float4 xx = *reinterpret_cast<const float4*>(x + i0);
  const float4 dv = ldv<NT, float4>(L.dv + i0);
  const uint32_t maxlen = max(max(ln.x, ln.y), max(ln.z, ln.w));
  float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  auto step = [&](uint32_t r0, uint32_t rmax) {
    float4 v[kU];
    float xg[kU][4];
    gather_group<D16, MODE, true, false, NT>(L, x, i0, r0, rmax, ln, v, xg);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t r = r0 + u;
        if (r == u4(dr, k)) ax[k] += f4(dv, k) * f4(xx, k);
        if (r < u4(ln, k)) ax[k] += f4(v[u], k) * xg[u][k];
      }
  };
  uint32_t r0 = 0;
  if constexpr (MODE != 0) {
    step(0, (uint32_t)max(L.w, 1) - 1u);  // peeled first group (see k_amg_smooth)
    r0 = kU;
  }
  for (; r0 < maxlen; r0 += kU) step(r0, maxlen - 1u);
  // a diagonal ranked after every visited slot (rank = len >= r0) comes last
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (u4(dr, k) >= r0) ax[k] += f4(dv, k) * f4(xx, k);
  const float4 bb = ldv<NT, float4>(b + i0);
  float4 o;
  o.x = bb.x - ax[0];
  o.y = bb.y - ax[1];
  o.z = bb.z - ax[2];
  o.w = bb.w - ax[3];
  return o;
}
template <bool D16, int MODE, bool NT = false>
__global__ void __launch_bounds__(kBlock) k_amg_residual(AmgLevelDev L, const float* __restrict__ x,
                                                         const float* __restrict__ b, float* __restrict__ rr) {
  uint32_t i0;
  if (!row_range<kRevResidual>(L.r0, L.r1, L.r2, L.r3, i0)) return;
  *reinterpret_cast<float4*>(rr + i0) = residual4<D16, MODE, NT>(L, x, b, i0);
}

// coarse value I of the restriction: sum_{f in R row I, ascending} 1.0 * r[f]
__device__ __forceinline__ float restrict_sum(const AmgLevelDev& L, const float* __restrict__ r, uint32_t I) {
  float sum = 0.0f;
  if (L.r_m4) {
    // the first 4 members in one 16-byte load, then their values
    const int4 m = L.r_m4[I];
    const bool over = m.w < -1;  // more than 4 members: member 3 stored as -2 - f
    const int f[4] = {m.x, m.y, m.z, over ? -2 - m.w : m.w};
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = r[max(f[q], 0)];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (f[q] >= 0) sum += 1.0f * v[q];
    if (over)  // the members after the fourth, in ascending order
      for (uint32_t k = L.r_row[I] + 4; k < L.r_row[I + 1]; ++k) sum += 1.0f * r[L.r_col[k]];
  } else {
    // members fetched 4 at a time (indices clamped to the row's last member,
    // unused values skipped): one round trip for the indices and one for the
    // values per 4 members instead of one dependent pair per member
    const uint32_t k0 = L.r_row[I], k1 = L.r_row[I + 1];
    for (uint32_t k = k0; k < k1; k += 4) {
      uint32_t f[4];
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) f[q] = L.r_col[min(k + q, k1 - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = r[f[q]];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k + q < k1) sum += 1.0f * v[q];
    }
  }
  return sum;
}

// restriction part: coarse_b[I] = sum_{f in R row I, ascending} 1.0 * r[f];
// also clears the coarse solution (amg.rs:721-725 `clear`, fused), including
// its ghost entries [-glo, 0) and [stride_c, stride_c + ghi) on a distributed level
__global__ void __launch_bounds__(kBlock) k_amg_restrict(AmgLevelDev L, const float* __restrict__ r,
                                                         float* __restrict__ cb,
                                                         float* __restrict__ cx, uint32_t stride_c,
                                                         uint32_t glo, uint32_t ghi,
                                                         float* __restrict__ sm_out,
                                                         const float* __restrict__ sm_de, uint32_t I0,
                                                         uint32_t I1) {
  const uint32_t I = I0 + row_id();
  if (I < I1) {
    // the coarse diagonal loaded with the members (no round trip after the sum)
    const float dec = sm_out ? sm_de[I] : 1.0f;
    const float sum = restrict_sum(L, r, I);
    cb[I] = sum;
    if (sm_out)  // the coarse level's zero-x pre-smoother fused (k_amg_smooth_zero)
      sm_out[I] = wmix(0.0f, (sum - 0.0f) / dec, 0.8f);
    else
      cx[I] = 0.0f;
    return;
  }
  if (sm_out) return;
  const uint32_t g = I - I1;
  if (g < glo)
    cx[-1 - (int)g] = 0.0f;
  else if (g < glo + ghi)
    cx[stride_c + (g - glo)] = 0.0f;
}

// Residual (amg.wgsl:80-111) and restriction (:114-120) of a single-GPU or
// replicated level in one kernel: a block owns aggregates [I0, I1) (L.rr_agg
// per block); its threads compute the residuals of those aggregates' members,
// rows r_col[p] for p in [r_row[I0], r_row[I1]), one row per thread, into
// LDS in member order; then thread t sums aggregate I0 + t's members in
// ascending order.  Every row's residual accumulates as in k_amg_residual
// (slots below the diagonal's rank, the diagonal, the rest) and every coarse
// value as in k_amg_restrict (0 + r_1 + r_2 ...): the same f32 operations.
// Saves the residual vector's store and the restriction's gathers of it, and
// one launch per level.  Bottom-up (kRevResidual), after the top-down smoother.
template <bool D16>
__global__ void __launch_bounds__(kBlock) k_amg_resrestrict(AmgLevelDev L, const float* __restrict__ x,
                                                            const float* __restrict__ b, float* __restrict__ cb,
                                                            float* __restrict__ cx, float* __restrict__ sm_out,
                                                            const float* __restrict__ sm_de) {
  __shared__ float rl[kRRCap];
  const uint32_t I0 = xcd_block<kRevResidual>() * L.rr_agg;
  if (I0 >= L.nc) return;
  const uint32_t I1 = min(I0 + L.rr_agg, L.nc);
  const uint32_t p0 = L.r_row[I0], p1 = L.r_row[I1];
  const uint32_t w = (uint32_t)max(L.w, 1);
  // this thread's aggregate's member range and coarse diagonal, loaded before
  // the residual phase (no dependent round trips after the barrier)
  [[maybe_unused]] uint32_t mk0 = 0, mk1 = 0;
  [[maybe_unused]] float dec = 1.0f;
  if (I0 + threadIdx.x < I1) {
    mk0 = L.r_row[I0 + threadIdx.x];
    mk1 = L.r_row[I0 + threadIdx.x + 1];
    if (sm_out) dec = sm_de[I0 + threadIdx.x];
  }
  for (uint32_t p = p0 + threadIdx.x; p < p1; p += kBlock) {
    const uint32_t f = L.r_col[p];
    const uint32_t len = L.len[f], dr = L.drank[f];
    const float xf = x[f], dvf = L.dv[f];
    float ax = 0.0f;
    uint32_t r0 = 0;
    for (; r0 < len; r0 += 4) {
      float v[4], xg[4];
      int c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t off = (size_t)min(r0 + u, w - 1u) * L.stride + f;
        v[u] = L.val[off];
        c[u] = D16 ? (int)f + (int)L.col16[off] : L.col32[off];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xg[u] = x[c[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t r = r0 + u;
        if (r == dr) ax += dvf * xf;
        if (r < len) ax += v[u] * xg[u];
      }
    }
    if (dr >= r0) ax += dvf * xf;  // a diagonal ranked after every visited slot comes last
    rl[p - p0] = b[f] - ax;
  }
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (I0 + t >= I1) return;
  const uint32_t I = I0 + t;
  float sum = 0.0f;
  for (uint32_t k = mk0; k < mk1; ++k) sum += 1.0f * rl[k - p0];
  cb[I] = sum;
  if (sm_out)  // the coarse level's zero-x pre-smoother fused (k_amg_smooth_zero)
    sm_out[I] = wmix(0.0f, (sum - 0.0f) / dec, 0.8f);
  else
    cx[I] = 0.0f;
}

// The up-leg of two adjacent single-GPU / replicated levels (c, c-1) in one
// launch (AmgUpPairImage, kernels.hpp): phase 1 smooths the level-c rows T
// the block needs with their prolongation from level c+1 applied to every
// read (k_amg_smooth<..., PRO>'s operations: x' = x + (0 + 1 x_c+1[agg]),
// sigma over the off-diagonals in slot order, mix(x', (b - sigma) / de,
// 0.8)) into LDS; phase 2 smooths the block's fine rows the same way with
// x_f + (0 + 1 x_c[agg]) read from that LDS image.  The fine rows' slots,
// columns, local indices and x gathers are loaded before phase 1.
template <bool D16F, bool D16C>
__global__ void __launch_bounds__(kUpPairRows) k_amg_prolong_smooth_pair(AmgLevelDev Lf, AmgLevelDev Lc,
                                                                       AmgUpPairImage P,
                                                                       const float* __restrict__ xf,
                                                                       const float* __restrict__ bf,
                                                                       float* __restrict__ xf_out,
                                                                       const float* __restrict__ xc,
                                                                       const float* __restrict__ bc,
                                                                       const float* __restrict__ xcc) {
  __shared__ float xs[kUpPairCap];
  const uint32_t blk = xcd_block<kRevSmooth>();
  if (blk >= P.nblocks) return;
  const uint32_t t = threadIdx.x;
  const uint32_t f = blk * kUpPairRows + t;
  const bool own = f < Lf.n;
  // fine row operands (independent of phase 1)
  constexpr int W = kPairW;
  uint32_t flen = 0, flo = 0;
  float fx = 0.0f, fb = 0.0f, fde = 1.0f;
  float fv[W], fg[W];
  uint32_t fl[W];
  const uint32_t wf = (uint32_t)max(Lf.w, 1);
  if (own) {
    flen = Lf.len[f];
    flo = P.lto[f];
    fx = xf[f];
    fb = bf[f];
    fde = Lf.de[f];
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const size_t off = (size_t)min((uint32_t)r, wf - 1u) * Lf.stride + f;
      fv[r] = Lf.val[off];
      fl[r] = P.lt[off];
      const int c = D16F ? (int)f + (int)Lf.col16[off] : Lf.col32[off];
      fg[r] = xf[c];
    }
  }
  // phase 1: post-smoothed level-c rows of T (prolongation from c+1 in the reads)
  const uint32_t t0 = P.tb[blk], nt = P.tb[blk + 1] - t0;
  const uint32_t wc = (uint32_t)max(Lc.w, 1);
  for (uint32_t q = t; q < nt; q += kUpPairRows) {
    const uint32_t g = P.t[t0 + q];
    const uint32_t len = Lc.len[g];
    float sg = 0.0f;
    for (uint32_t r = 0; r < len; ++r) {
      const size_t off = (size_t)min(r, wc - 1u) * Lc.stride + g;
      const int c = D16C ? (int)g + (int)Lc.col16[off] : Lc.col32[off];
      const float xg = prolonged(xc[c], xcc[Lc.agg[c]]);
      sg += Lc.val[off] * xg;
    }
    float xx = xc[g];
    float pc = 0.0f;
    pc += 1.0f * xcc[Lc.agg[g]];
    xx += pc;
    xs[q] = wmix(xx, (bc[g] - sg) / Lc.de[g], 0.8f);
  }
  __syncthreads();
  // phase 2: the block's fine rows, x_f + P x_c read through the LDS image
  if (!own) return;
  float sg = 0.0f;
  for (uint32_t r = 0; r < flen; ++r) {
    float v, xg;
    if (r < (uint32_t)W) {
      v = fv[r];
      xg = prolonged(fg[r], xs[fl[r]]);
    } else {
      const size_t off = (size_t)r * Lf.stride + f;
      const int c = D16F ? (int)f + (int)Lf.col16[off] : Lf.col32[off];
      v = Lf.val[off];
      xg = prolonged(xf[c], xs[P.lt[off]]);
    }
    sg += v * xg;
  }
  float pc = 0.0f;
  pc += 1.0f * xs[flo];
  fx += pc;
  xf_out[f] = wmix(fx, (fb - sg) / fde, 0.8f);
}

// The down-leg of two adjacent single-GPU / replicated levels (i, i+1) in one
// launch (AmgPairImage, kernels.hpp): the two k_amg_resrestrict launches'
// arithmetic, operation for operation.  Phase 1: one level-i member residual
// per thread (k_amg_resrestrict's loop) into LDS; phase 2: every S row's rhs
// (0 + r_1 + r_2 ... in R order) and its zero-x pre-smoother
// mix(0, (b - 0) / de, 0.8), the block's own rows stored; phase 3: the level-
// (i+1) residual of the block's rows from the LDS values (diagonal at its rank
// among the off-diagonals, as k_amg_resrestrict); phase 4: the level-(i+2)
// rhs per aggregate and its pre-smoother (or x = 0).  The level-(i+1) slots,
// row headers and the aggregate ranges are loaded before phase 1, so the
// second level costs LDS round trips only; the ring rows' level-i residuals
// are the redundant work (amg_fusion_ratio.py).
template <bool D16, uint32_t NTH>
__global__ void __launch_bounds__(NTH) k_amg_resrestrict_pair(AmgLevelDev Lf, AmgLevelDev Lm,
                                                                     AmgPairImage P, const float* __restrict__ x,
                                                                     const float* __restrict__ b,
                                                                     float* __restrict__ bm, float* __restrict__ xm,
                                                                     float* __restrict__ cb, float* __restrict__ cx,
                                                                     float* __restrict__ sm_out,
                                                                     const float* __restrict__ sm_de) {
  __shared__ float rl[NTH];  // level-i residuals of the block's f rows
  __shared__ float bs[NTH];  // level-(i+1) rhs of the block's s rows
  __shared__ float xs[NTH];  // their pre-smoothed x
  __shared__ float r2[NTH];  // level-(i+1) residuals of the block's own rows
  const uint32_t blk = xcd_block<kRevResidual>();
  if (blk >= P.nblocks) return;
  const uint32_t t = threadIdx.x;
  const uint32_t s0 = P.sb[blk], s1 = P.sb[blk + 1];
  const uint32_t J0 = P.jb[blk], J1 = P.jb[blk + 1];
  const uint32_t m0 = Lm.r_row[J0], nm = Lm.r_row[J1] - m0;
  const uint32_t fb = P.fo[s0], fe = P.fo[s1];
  // phase-2 / phase-3 / phase-4 operands, independent of phase 1
  uint32_t sr = 0, k0 = 0, k1 = 0, mlen = 0, mdr = 0, a0 = 0, a1 = 0;
  float des = 1.0f, mdv = 0.0f, dec = 1.0f;
  float mv[kPairW];
  uint32_t mc[kPairW];
  if (s0 + t < s1) {
    sr = P.s[s0 + t];
    k0 = P.fo[s0 + t];
    k1 = P.fo[s0 + t + 1];
    des = Lm.de[sr];
  }
  if (t < nm) {
    mlen = Lm.len[sr];
    mdr = Lm.drank[sr];
    mdv = Lm.dv[sr];
    const uint32_t wm = (uint32_t)max(Lm.w, 1);
#pragma unroll
    for (int r = 0; r < kPairW; ++r) {
      const size_t off = (size_t)min((uint32_t)r, wm - 1u) * Lm.stride + sr;
      mv[r] = Lm.val[off];
      mc[r] = P.lc[off];
    }
  }
  if (J0 + t < J1) {
    a0 = Lm.r_row[J0 + t];
    a1 = Lm.r_row[J0 + t + 1];
    if (sm_out) dec = sm_de[J0 + t];
  }
  // phase 1: level-i residuals (k_amg_resrestrict's row loop)
  const uint32_t w = (uint32_t)max(Lf.w, 1);
  for (uint32_t p = fb + t; p < fe; p += NTH) {
    const uint32_t f = P.f[p];
    const uint32_t len = Lf.len[f], dr = Lf.drank[f];
    const float xf = x[f], dvf = Lf.dv[f];
    float ax = 0.0f;
    uint32_t r0 = 0;
    for (; r0 < len; r0 += 4) {
      float v[4], xg[4];
      int c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t off = (size_t)min(r0 + u, w - 1u) * Lf.stride + f;
        v[u] = Lf.val[off];
        c[u] = D16 ? (int)f + (int)Lf.col16[off] : Lf.col32[off];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xg[u] = x[c[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t r = r0 + u;
        if (r == dr) ax += dvf * xf;
        if (r < len) ax += v[u] * xg[u];
      }
    }
    if (dr >= r0) ax += dvf * xf;
    rl[p - fb] = b[f] - ax;
  }
  __syncthreads();
  // phase 2: level-(i+1) rhs (restriction) and zero-x pre-smoother of every s row
  if (s0 + t < s1) {
    float sum = 0.0f;
    for (uint32_t k = k0; k < k1; ++k) sum += 1.0f * rl[k - fb];
    const float xv = wmix(0.0f, (sum - 0.0f) / des, 0.8f);
    bs[t] = sum;
    xs[t] = xv;
    if (t < nm) {  // the block's own rows (every level-(i+1) row is one block's)
      bm[sr] = sum;
      xm[sr] = xv;
    }
  }
  __syncthreads();
  // phase 3: level-(i+1) residual of the block's rows
  if (t < nm) {
    const float xf = xs[t];
    float ax = 0.0f;
    uint32_t r = 0;
    for (; r < mlen; ++r) {
      float v;
      uint32_t c;
      if (r < (uint32_t)kPairW) {
        v = mv[r];
        c = mc[r];
      } else {
        const size_t off = (size_t)r * Lm.stride + sr;
        v = Lm.val[off];
        c = P.lc[off];
      }
      if (r == mdr) ax += mdv * xf;
      ax += v * xs[c];
    }
    if (mdr >= r) ax += mdv * xf;  // a diagonal ranked after every off-diagonal comes last
    r2[t] = bs[t] - ax;
  }
  __syncthreads();
  // phase 4: level-(i+2) rhs (restriction) and its pre-smoother / cleared x
  if (J0 + t < J1) {
    const uint32_t J = J0 + t;
    float sum = 0.0f;
    for (uint32_t k = a0; k < a1; ++k) sum += 1.0f * r2[k - m0];
    cb[J] = sum;
    if (sm_out)
      sm_out[J] = wmix(0.0f, (sum - 0.0f) / dec, 0.8f);
    else
      cx[J] = 0.0f;
  }
}

// prolongate_op (amg.wgsl:56-75): x += (0 + 1 * xc[agg]), 4 rows per thread.
// agg is a signed local index on a distributed level (aggregates seeded on a
// lower rank are ghosts of xc below 0).
template <bool NT>
__global__ void __launch_bounds__(kBlock) k_amg_prolong(AmgLevelDev L, float* __restrict__ x,
                                                        const float* __restrict__ xc, uint32_t f0, uint32_t f1) {
  const uint32_t i0 = f0 + 4 * row_id();
  if (i0 >= f1) return;
  float4 xx = *reinterpret_cast<const float4*>(x + i0);
  const int4 ag = ldv<NT, int4>(L.agg + i0);
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;  // padding rows (>= n) get 0
  c0 += 1.0f * xc[ag.x];
  if (i0 + 1 < L.n) c1 += 1.0f * xc[ag.y];
  if (i0 + 2 < L.n) c2 += 1.0f * xc[ag.z];
  if (i0 + 3 < L.n) c3 += 1.0f * xc[ag.w];
  xx.x += c0;
  xx.y += c1;
  xx.z += c2;
  xx.w += c3;
  *reinterpret_cast<float4*>(x + i0) = xx;
}

}  // namespace

// instance for a level: 16/32-bit columns x load mode (see gather_group) x load policy
#define CFD_AMG_INSTANCE(kern, L, ...)                                                  \
  ((L).use16 ? ((L).full ? kern<true, 1, __VA_ARGS__> : kern<true, 0, __VA_ARGS__>) \
             : ((L).full ? kern<false, 1, __VA_ARGS__> : kern<false, 0, __VA_ARGS__>))

void launch_amg_smooth(const AmgLevelDev& L, const float* x, const float* b, float* x_out, hipStream_t s,
                       hipEvent_t ev0, hipEvent_t ev1, bool nt) {
  if (L.r1 <= L.r0 && L.r3 <= L.r2) return;
  const unsigned nb = rows2_grid(L.r0, L.r1, L.r2, L.r3);
  auto fn = nt ? CFD_AMG_INSTANCE(k_amg_smooth, L, false, true) : CFD_AMG_INSTANCE(k_amg_smooth, L, false, false);
  if (ev0)  // timed launch: events recorded by the GPU at kernel start / end
    hipExtLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, ev0, ev1, 0, CFD_AMG_HEAD(L), x, b, x_out, L,
                          (const float*)nullptr);
  else
    hipLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, CFD_AMG_HEAD(L), x, b, x_out, L, (const float*)nullptr);
}
void launch_amg_smooth_ordered(const AmgLevelDev& L, float* x, const float* b, hipStream_t s) {
  if (L.n == 0) return;
  auto fn = L.use16 ? (L.full ? k_amg_smooth_ordered<true, 1> : k_amg_smooth_ordered<true, 0>)
                    : (L.full ? k_amg_smooth_ordered<false, 1> : k_amg_smooth_ordered<false, 0>);
  hipLaunchKernelGGL(fn, dim3(1), dim3(16), 0, s, L, x, b);
}
void launch_amg_smooth_prolong(const AmgLevelDev& L, const float* x, const float* xc, const float* b, float* x_out,
                               hipStream_t s) {
  if (L.r1 <= L.r0 && L.r3 <= L.r2) return;
  if (!L.agg || !xc) throw std::invalid_argument("amg_smooth_prolong: level without a coarse level");
  const unsigned nb = rows2_grid(L.r0, L.r1, L.r2, L.r3);
  auto fn = L.use16 ? (L.full ? k_amg_smooth<true, 1, true> : k_amg_smooth<true, 0, true>)
                    : (L.full ? k_amg_smooth<false, 1, true> : k_amg_smooth<false, 0, true>);
  hipLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, CFD_AMG_HEAD(L), x, b, x_out, L, xc);
}
void launch_amg_smooth_zero(const AmgLevelDev& L, const float* b, float* x_out, hipStream_t s) {
  if (L.n) hipLaunchKernelGGL(k_amg_smooth_zero, dim3(grid_for((L.n + 3) / 4)), dim3(kBlock), 0, s, L, b, x_out);
}
void launch_amg_residual(const AmgLevelDev& L, const float* x, const float* b, float* r, hipStream_t s, bool nt) {
  if (L.r1 <= L.r0 && L.r3 <= L.r2) return;
  const unsigned nb = rows2_grid(L.r0, L.r1, L.r2, L.r3);
  auto fn = nt ? CFD_AMG_INSTANCE(k_amg_residual, L, true) : CFD_AMG_INSTANCE(k_amg_residual, L, false);
  hipLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, L, x, b, r);
}
void launch_amg_restrict(const AmgLevelDev& L, const float* r, float* cb, float* cx, uint32_t stride_c,
                         uint32_t glo, uint32_t ghi, hipStream_t s, float* sm_out, const float* sm_de, uint32_t I0,
                         uint32_t I1, bool ghosts) {
  if (I1 == 0) I1 = L.nc;
  const size_t n = (size_t)(I1 - I0) + (sm_out || !ghosts ? 0 : (size_t)glo + ghi);
  if (n)
    hipLaunchKernelGGL(k_amg_restrict, dim3(grid_for(n)), dim3(kBlock), 0, s, L, r, cb, cx, stride_c, glo, ghi,
                       sm_out, sm_de, I0, I1);
}
void launch_amg_resrestrict(const AmgLevelDev& L, const float* x, const float* b, float* cb, float* cx,
                            float* sm_out, const float* sm_de, hipStream_t s) {
  if (!L.nc || !L.rr_agg) return;
  const unsigned nb = (unsigned)((L.nc + L.rr_agg - 1) / L.rr_agg);
  if (L.use16)
    hipLaunchKernelGGL(k_amg_resrestrict<true>, dim3(nb), dim3(kBlock), 0, s, L, x, b, cb, cx, sm_out, sm_de);
  else
    hipLaunchKernelGGL(k_amg_resrestrict<false>, dim3(nb), dim3(kBlock), 0, s, L, x, b, cb, cx, sm_out, sm_de);
}
void launch_amg_prolong_smooth_pair(const AmgLevelDev& Lf, const AmgLevelDev& Lc, const AmgUpPairImage& P,
                                    const float* xf, const float* bf, float* xf_out, const float* xc,
                                    const float* bc, const float* xcc, hipStream_t s) {
  if (!P.nblocks) return;
  auto fn = Lf.use16 ? (Lc.use16 ? k_amg_prolong_smooth_pair<true, true> : k_amg_prolong_smooth_pair<true, false>)
                     : (Lc.use16 ? k_amg_prolong_smooth_pair<false, true> : k_amg_prolong_smooth_pair<false, false>);
  hipLaunchKernelGGL(fn, dim3(P.nblocks), dim3(kUpPairRows), 0, s, Lf, Lc, P, xf, bf, xf_out, xc, bc, xcc);
}
void launch_amg_resrestrict_pair(const AmgLevelDev& Lf, const AmgLevelDev& Lm, const AmgPairImage& P,
                                 const float* x, const float* b, float* bm, float* xm, float* cb, float* cx,
                                 float* sm_out, const float* sm_de, hipStream_t s) {
  if (!P.nblocks) return;
  auto fn = P.threads == 256 ? (Lf.use16 ? k_amg_resrestrict_pair<true, 256> : k_amg_resrestrict_pair<false, 256>)
                             : (Lf.use16 ? k_amg_resrestrict_pair<true, kPairThreads>
                                         : k_amg_resrestrict_pair<false, kPairThreads>);
  hipLaunchKernelGGL(fn, dim3(P.nblocks), dim3(P.threads), 0, s, Lf, Lm, P, x, b, bm, xm, cb, cx, sm_out, sm_de);
}
void launch_amg_prolong(const AmgLevelDev& L, float* x, const float* xc, hipStream_t s, uint32_t f0, uint32_t f1, bool nt) {
  if (f1 == 0) f1 = L.n;
  if (f1 > f0)
    hipLaunchKernelGGL(nt ? k_amg_prolong<true> : k_amg_prolong<false>, dim3(grid_for((f1 - f0 + 3) / 4)), dim3(kBlock), 0, s, L, x, xc, f0, f1);
}

}  // namespace cfd2
