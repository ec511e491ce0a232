// Row kernels of the coupled matrix (2 cells per thread): SpMV and the Schur
// preconditioner's predict / correct, with its relax_pressure sweeps.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "amg_rows.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// Slot-group sizes of the coupled row kernels (all loads of a group are
// issued before the first use).  Build-time tunables (tools/ab_variants.py).
#ifndef CFD_SPMV_U
#define CFD_SPMV_U 4
#endif
#ifndef CFD_PREDICT_U
#define CFD_PREDICT_U 4
#endif
#ifndef CFD_CORRECT_U
#define CFD_CORRECT_U 4
#endif

// Slot loads of the row kernels are unconditional: slot r reads ELL slot
// min(r, ws - 1) (ws = the matrix's ELL width, kernel-uniform), which always
// exists; unused slots hold value 0 and the row's own column, and every
// accumulation skips r >= len, so results are unchanged.  Without a branch
// per slot the compiler issues a whole group's matrix loads back to back
// (a predicated load per slot made it wait for each slot's column load
// before issuing the next slot), and the first group does not wait for the
// row lengths.  The first group (U1) is sized to cover a whole interior row
// (5 entries of a quad cell's coupled row).
// SpMV: the first slot group's cval_a / cval_g loads are issued with the row
// headers, before the wait for them (C2 216 -> 197 us; the same for the
// Schur prediction lost 150 -> 158 us: profiles/r03/ab_coupled_pre_c2.txt;
// the regular rows' x gathers issued speculatively as well gained nothing
// more, 198 -> 200 us: ab_spmv_spec_c2.txt)
#ifndef CFD_SPMV_U1
#define CFD_SPMV_U1 5
#endif

// The coupled row kernels (SpMV, Schur predict / correct) take 2 cells (6
// rows) per thread: half the registers per slot group of the 4-cell form
// (102 instead of 196 VGPRs: 4 wavefronts per SIMD instead of 2), one 16-byte
// load per slot array; same-box A/B at C2 (round 2): SpMV 225.8 -> 218.0 us.
template <bool REV = false>
__device__ __forceinline__ bool row_range2(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t& i0) {
  const uint32_t t = row_id<REV>(), na = (r1 - r0 + 1) / 2;
  if (t < na) {
    i0 = r0 + 2 * t;
    return i0 < r1;
  }
  i0 = r2 + 2 * (t - na);
  return i0 < r3;
}
inline unsigned rows2x_grid(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
  const size_t t = (size_t)(r1 - r0 + 1) / 2 + (r3 > r2 ? (size_t)(r3 - r2 + 1) / 2 : 0);
  return (unsigned)((t + 255) / 256);
}
// the two rows' columns of slot offset `off`
template <bool D16, bool NT = false>
__device__ __forceinline__ void ccols2(const CoupledMatrix& A, size_t off, uint32_t i0, int c[2]) {
  if constexpr (D16) {
    const short2 d = ldv<NT, short2>(A.col16 + off);
    c[0] = (int)i0 + (int)d.x;
    c[1] = (int)i0 + 1 + (int)d.y;
  } else {
    const int2 q = ldv<NT, int2>(A.col + off);
    c[0] = q.x;
    c[1] = q.y;
  }
}
__device__ __forceinline__ bool lg2_on(uint32_t w, uint32_t r) { return r < (w & kLgUsedMask) && !((w >> 8 >> r) & 1u); }
// REG (first slot group of a wave of regular rows, r0 = 0): columns
// row + tmode[slot] (no column loads), and the two rows' x entries are six
// consecutive floats (one 16-byte + one 8-byte gather)
// PRE: the group's cval_a / cval_g slots were loaded by the caller (first
// group: issued right after the row headers, before the wait for them)
template <bool D16, int U, bool REG = false, bool PRE = false, bool NT = false>
__device__ __forceinline__ void spmv2_group(const CoupledMatrix& A, const float* __restrict__ x, uint32_t i0,
                                            uint32_t r0, uint32_t rmax, const uint32_t lw[2], const uint32_t dr[2],
                                            const float2 d2[2], float su[2], float sv[2], float sp[2],
                                            const float4* pa = nullptr, const float4* pg = nullptr) {
  float4 a[U], g[U];
  int c[U][2];
  float xg[U][2][3];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t off = (size_t)min(r0 + u, rmax) * A.ld + i0;
    if constexpr (PRE) {
      a[u] = pa[u];
      g[u] = pg[u];
    } else {
      a[u] = ldv<NT, float4>(A.cval_a + off);
      g[u] = ldv<NT, float4>(A.cval_g + off);
    }
    if constexpr (REG) {
      c[u][0] = (int)i0 + A.tmode[u];
      c[u][1] = c[u][0] + 1;
    } else {
      ccols2<D16, NT>(A, off, i0, c[u]);
    }
  }
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* b = x + 3 * (ptrdiff_t)c[u][0];
      const f4u q0 = ld4u(b);
      const f2u q1 = ld2u(b + 4);
      xg[u][0][0] = q0.x;
      xg[u][0][1] = q0.y;
      xg[u][0][2] = q0.z;
      xg[u][1][0] = q0.w;
      xg[u][1][1] = q1.x;
      xg[u][1][2] = q1.y;
    }
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const ptrdiff_t j = 3 * (ptrdiff_t)c[u][k];
        xg[u][k][0] = x[j];
        xg[u][k][1] = x[j + 1];
        xg[u][k][2] = x[j + 2];
      }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t r = r0 + u;
      if (!lg2_on(lw[k], r)) continue;
      const bool dg = (r == dr[k]);
      const float uu = k ? a[u].z : a[u].x, pp = k ? a[u].w : a[u].y;
      const float up = k ? g[u].z : g[u].x, vp = k ? g[u].w : g[u].y;
      const float pu = dg ? d2[k].x : up, pv = dg ? d2[k].y : vp;
      const float xu = xg[u][k][0], xv = xg[u][k][1], xp = xg[u][k][2];
      su[k] += uu * xu;
      su[k] += 0.0f * xv;
      su[k] += up * xp;
      sv[k] += 0.0f * xu;
      sv[k] += uu * xv;
      sv[k] += vp * xp;
      sp[k] += pu * xu;
      sp[k] += pv * xv;
      sp[k] += pp * xp;
    }
}
// the two rows' slot headers (u16) and diagonal slots (u8).  Packing both
// into one u32 per row (one load fewer) lost at C2: SpMV 208 -> 213, Schur
// prediction 155 -> 160 us (profiles/r03/ab_log.md) -- 2 bytes more per row
// cost more than the instruction saved.
template <bool NT = false>
__device__ __forceinline__ void row2_headers(const CoupledMatrix& A, uint32_t i0, uint32_t lw[2], uint32_t dr[2]) {
  const ushort2 lg = ldv<NT, ushort2>(A.lg + i0);
  const uchar2 drr = ldv<NT, uchar2>(A.drank + i0);
  lw[0] = lg.x;
  lw[1] = lg.y;
  dr[0] = drr.x;
  dr[1] = drr.y;
}
// b != null: y = 1 * b + -1 * (A x), the residual's axpby (gmres_ops.wgsl:108-117)
// applied to each output element as it is stored (compute_residual_into: the
// product itself is not needed)
template <bool D16, bool NT>
__global__ void __launch_bounds__(kBlock) k_spmv2(CoupledMatrix A, const float* __restrict__ x,
                                                  float* __restrict__ y, const float* __restrict__ b) {
  constexpr int U = CFD_SPMV_U, U1 = CFD_SPMV_U1;
  uint32_t i0;
  if (!row_range2<kRevSpmv>(A.r0, A.r1, A.r2, A.r3, i0)) return;
  uint32_t lw[2], dr[2];
  row2_headers<NT>(A, i0, lw, dr);
  const float4 dd = ldv<NT, float4>(A.cdiag2 + i0);
  const float2 d2[2] = {make_float2(dd.x, dd.y), make_float2(dd.z, dd.w)};
  const uint32_t maxlen = max(lw[0] & kLgUsedMask, lw[1] & kLgUsedMask);
  float su[2] = {0.0f, 0.0f}, sv[2] = {0.0f, 0.0f}, sp[2] = {0.0f, 0.0f};
  // the first slot group's values issued with the row headers (see CFD_SPMV_U1)
  float4 pa[U1], pg[U1];
#pragma unroll
  for (int u = 0; u < U1; ++u) {
    const size_t off = (size_t)min((uint32_t)u, (uint32_t)A.ws - 1u) * A.ld + i0;
    pa[u] = ldv<NT, float4>(A.cval_a + off);
    pg[u] = ldv<NT, float4>(A.cval_g + off);
  }
  if (A.reg && A.ws <= U1 && __all((lw[0] & lw[1] & kLgRegular) != 0u))  // ws <= U1: the only group
    spmv2_group<D16, U1, true, true, NT>(A, x, i0, 0, (uint32_t)A.ws - 1u, lw, dr, d2, su, sv, sp, pa, pg);
  else
    spmv2_group<D16, U1, false, true, NT>(A, x, i0, 0, (uint32_t)A.ws - 1u, lw, dr, d2, su, sv, sp, pa, pg);
  for (uint32_t r0 = U1; r0 < maxlen; r0 += U)
    spmv2_group<D16, U, false, false, NT>(A, x, i0, r0, maxlen - 1u, lw, dr, d2, su, sv, sp);
  float* yo = y + 3 * (size_t)i0;  // 8-byte aligned (i0 even)
  typedef float f2v __attribute__((ext_vector_type(2)));
  if (b) {
    const float* bo = b + 3 * (size_t)i0;
    const f4u b4 = ldv<NT, f4u>(bo);
    const f2u b2 = ldv<NT, f2u>(bo + 4);
    *reinterpret_cast<f4u*>(yo) = f4u{1.0f * b4.x + -1.0f * su[0], 1.0f * b4.y + -1.0f * sv[0],
                                      1.0f * b4.z + -1.0f * sp[0], 1.0f * b4.w + -1.0f * su[1]};
    *reinterpret_cast<f2v*>(yo + 4) = f2v{1.0f * b2.x + -1.0f * sv[1], 1.0f * b2.y + -1.0f * sp[1]};
    return;
  }
  *reinterpret_cast<f4u*>(yo) = f4u{su[0], sv[0], sp[0], su[1]};
  *reinterpret_cast<f2v*>(yo + 4) = f2v{sv[1], sp[1]};
}

#ifndef CFD_PREDICT_U1
#define CFD_PREDICT_U1 5
#endif

// Every relax_pressure sweep of one preconditioner application in ONE
// workgroup (small meshes, N < 8192): the p_iters launches of k_relax_pressure4
// (64 at the reference's 8 k-cell benchmark mesh, each a ~4.6 us launch for a
// few microseconds of work) become one kernel.  Thread t owns rows t + 1024 k;
// its rows' off-diagonal entries (values + LDS byte addresses of their
// columns, compacted in slot order: the diagonal is skipped as in
// k_relax_pressure4), temp_p and dinv_p live in registers for all sweeps; the
// two ping-pong iterates live in LDS (P = p_sol at byte 0, T = temp at byte
// 32768: a sweep's source buffer is an immediate offset; unit-stride rows keep
// the neighbour reads free of bank conflicts).  Sweep s reads the iterate
// written by sweep s-1 (P for even s, T for odd) and writes the other buffer,
// exactly the launch sequence's src/dst alternation; one barrier per sweep
// orders it.  Unused entries point at a zero row with value +0: they add
// +0 * +0 = +0 to sigma, which starts at +0 and so is never -0 (a
// round-to-nearest sum is -0 only if both operands are), hence sigma + +0 ==
// sigma bit for bit -- the f32 result of k_relax_pressure4, without a compare
// and select per entry.
constexpr int kRelaxThreads = 1024;
template <int RPT, int OD>
__global__ void __launch_bounds__(kRelaxThreads) k_relax_pressure_fused(uint32_t N, uint32_t ld,
                                                                      const int32_t* __restrict__ col,
                                                                      const uint32_t* __restrict__ len,
                                                                      const float* __restrict__ sval,
                                                                      const float* __restrict__ dinv_p,
                                                                      const float* __restrict__ temp_p,
                                                                      float* p_sol, float* temp, uint32_t iters) {
  extern __shared__ float relax_lds[];  // P [0, 8192), T [8192, 16384); row N of each = +0
  char* base = reinterpret_cast<char*>(relax_lds);
  constexpr uint32_t kT = 4u * kRelaxFusedMaxRows + 4u;  // byte offset of T (32768)
  const uint32_t t = threadIdx.x;
  float dv[RPT], tp[RPT], v[RPT][OD];
  // own rows of both iterates (P: own[0], T: own[1]) also live in registers:
  // a sweep's mix operand (the destination's previous value, written by this
  // thread two sweeps earlier) is read from them, not from LDS
  float own[2][RPT];
  uint32_t ad[RPT][OD];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const uint32_t i = t + (uint32_t)k * kRelaxThreads;
    dv[k] = tp[k] = own[0][k] = own[1][k] = 0.0f;
#pragma unroll
    for (int e = 0; e < OD; ++e) {
      v[k][e] = 0.0f;
      ad[k][e] = 4u * N;  // the zero row
    }
    if (i < N) {
      own[0][k] = relax_lds[i] = p_sol[i];
      own[1][k] = relax_lds[kT / 4 + i] = temp[i];
      dv[k] = dinv_p[i];
      tp[k] = temp_p[i];
      const uint32_t l = len[i];
      int e = 0;
#pragma unroll
      for (int r = 0; r <= OD; ++r) {  // <= OD off-diagonals + the diagonal
        if ((uint32_t)r < l) {
          const size_t slot = (size_t)r * ld + i;
          const int32_t cc = col[slot];
          if (cc != (int32_t)i) {
            // e only ever increases by one: a static select chain keeps v / ad in registers
#pragma unroll
            for (int q = 0; q < OD; ++q)
              if (q == e) {
                v[k][q] = sval[slot];
                ad[k][q] = 4u * (uint32_t)cc;
              }
            ++e;
          }
        }
      }
    }
  }
  if (t == 0) relax_lds[N] = relax_lds[kT / 4 + N] = 0.0f;
  __syncthreads();
  // SRC = byte offset of the source iterate (0: P, kT: T)
  auto sweep = [&](auto src_off) {
    constexpr uint32_t SRC = decltype(src_off)::value, DST = kT - SRC;
    constexpr int DI = DST == 0 ? 0 : 1;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      // rows past N compute on the zero row: +0 entries, dv = tp = own = +0, so
      // they write mix(+0, +0, 1.2) = +0 back into it (branch-free sweep)
      const uint32_t i = min(t + (uint32_t)k * kRelaxThreads, N);
      float sigma = 0.0f;
#pragma unroll
      for (int e = 0; e < OD; ++e) sigma += v[k][e] * *reinterpret_cast<const float*>(base + ad[k][e] + SRC);
      const float hat_x = dv[k] * (tp[k] - sigma);
      // own row: only this thread touches it in this sweep
      own[DI][k] = wmix(own[DI][k], hat_x, 1.2f);
      *reinterpret_cast<float*>(base + 4u * i + DST) = own[DI][k];
    }
    __syncthreads();
  };
  uint32_t s = 0;
  for (; s + 1 < iters; s += 2) {
    sweep(std::integral_constant<uint32_t, 0u>{});
    sweep(std::integral_constant<uint32_t, kT>{});
  }
  if (s < iters) sweep(std::integral_constant<uint32_t, 0u>{});
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const uint32_t i = t + (uint32_t)k * kRelaxThreads;
    if (i < N) {
      p_sol[i] = own[0][k];
      temp[i] = own[1][k];
    }
  }
}

#ifndef CFD_CORRECT_U1
#define CFD_CORRECT_U1 5
#endif

// ---- Schur predict / correct, 2 cells per thread ----
// The row operands of the Schur kernels are loaded with the row header, not
// after the slot loop: the prediction's dinv_p, the correction's V_j,
// dinv_uv and own p_sol -- one dependent round trip fewer per wave.
// Same-box A/B at C2 (profiles/r03/ab_rev_schur_early_c2.txt): prediction
// 152.3 -> 144.9, correction 135.8 -> 132.4 us, 254.8 -> 253.1 ms/step;
// C1 39.95 -> 39.22.
template <bool D16, int U, bool REG = false, bool NT = false>  // REG: see spmv2_group
__device__ __forceinline__ void predict2_group(const CoupledMatrix& A, const float* __restrict__ w_in, float sc,
                                               const float* __restrict__ dinv_uv, uint32_t i0, uint32_t r0,
                                               uint32_t rmax, const uint32_t lw[2], const uint32_t dr[2],
                                               const float2 d2[2], float rhs[2]) {
  float4 g[U];
  int c[U][2];
  float gd[U][2], gu[U][2], gv[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t off = (size_t)min(r0 + u, rmax) * A.ld + i0;
    g[u] = ldv<NT, float4>(A.cval_g + off);
    if constexpr (REG) {
      c[u][0] = (int)i0 + A.tmode[u];
      c[u][1] = c[u][0] + 1;
    } else {
      ccols2<D16, NT>(A, off, i0, c[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {  // 2 consecutive cells: 8 + 24 bytes
    const f2u d = ld2u(dinv_uv + c[u][0]);
    const float* b = w_in + 3 * (ptrdiff_t)c[u][0];
    const f4u q0 = ld4u(b);
    const f2u q1 = ld2u(b + 4);
    gd[u][0] = d.x;
    gd[u][1] = d.y;
    gu[u][0] = q0.x;
    gv[u][0] = q0.y;
    gu[u][1] = q0.w;
    gv[u][1] = q1.x;
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (c[u][1] != c[u][0] + 1) {
      const ptrdiff_t j = 3 * (ptrdiff_t)c[u][1];
      gd[u][1] = dinv_uv[c[u][1]];
      gu[u][1] = w_in[j];
      gv[u][1] = w_in[j + 1];
    }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t r = r0 + u;
      if (!lg2_on(lw[k], r)) continue;
      const bool dg = (r == dr[k]);
      const float gx = k ? g[u].z : g[u].x, gy = k ? g[u].w : g[u].y;
      const float pu = dg ? d2[k].x : gx, pv = dg ? d2[k].y : gy;
      const float ru = sc * gu[u][k], rv = sc * gv[u][k];
      const float zu = ru * gd[u][k];
      const float zv = rv * gd[u][k];
      rhs[k] -= pu * zu;
      rhs[k] -= pv * zv;
    }
}
template <bool D16, bool NT>
__global__ void __launch_bounds__(kBlock) k_precond_predict2(CoupledMatrix A, const float* __restrict__ w_in,
                                                             const float* __restrict__ binv, int jv,
                                                             const float* __restrict__ dinv_uv,
                                                             const float* __restrict__ dinv_p, float* temp_p,
                                                             float* p_sol, float* p_prev) {
  constexpr int U = CFD_PREDICT_U, U1 = CFD_PREDICT_U1;
  uint32_t i0;
  if (!row_range2(A.r0, A.r1, A.r2, A.r3, i0)) return;
  const float sc = binv[jv];
  const float* wb = w_in + 3 * (size_t)i0;
  const f4u wa = ld4u(wb);
  const f2u wc = ld2u(wb + 4);
  float rhs[2] = {sc * wa.z, sc * wc.y};
  uint32_t lw[2], dr[2];
  row2_headers<NT>(A, i0, lw, dr);
  const float4 dd = ldv<NT, float4>(A.cdiag2 + i0);
  const float2 d2[2] = {make_float2(dd.x, dd.y), make_float2(dd.z, dd.w)};
  const float2 dp = ldv<NT, float2>(dinv_p + i0);
  const uint32_t maxlen = max(lw[0] & kLgUsedMask, lw[1] & kLgUsedMask);
  if (A.reg && A.ws <= U1 && __all((lw[0] & lw[1] & kLgRegular) != 0u))  // ws <= U1: the only group
    predict2_group<D16, U1, true, NT>(A, w_in, sc, dinv_uv, i0, 0, (uint32_t)A.ws - 1u, lw, dr, d2, rhs);
  else
    predict2_group<D16, U1, false, NT>(A, w_in, sc, dinv_uv, i0, 0, (uint32_t)A.ws - 1u, lw, dr, d2, rhs);
  for (uint32_t r0 = U1; r0 < maxlen; r0 += U)
    predict2_group<D16, U, false, NT>(A, w_in, sc, dinv_uv, i0, r0, maxlen - 1u, lw, dr, d2, rhs);
  *reinterpret_cast<float2*>(temp_p + i0) = make_float2(rhs[0], rhs[1]);
  *reinterpret_cast<float2*>(p_sol + i0) = make_float2(dp.x * rhs[0], dp.y * rhs[1]);
  if (p_prev) *reinterpret_cast<float2*>(p_prev + i0) = make_float2(0.0f, 0.0f);
}
template <bool D16, int U, bool REG = false>  // REG: see spmv2_group
__device__ __forceinline__ void correct2_group(const CoupledMatrix& A, const float* __restrict__ p_sol, uint32_t i0,
                                               uint32_t r0, uint32_t rmax, const uint32_t lw[2], float cu[2],
                                               float cv[2]) {
  float4 g[U];
  int c[U][2];
  float pj[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t off = (size_t)min(r0 + u, rmax) * A.ld + i0;
    g[u] = *reinterpret_cast<const float4*>(A.cval_g + off);
    if constexpr (REG) {
      c[u][0] = (int)i0 + A.tmode[u];
      c[u][1] = c[u][0] + 1;
    } else {
      ccols2<D16>(A, off, i0, c[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f2u q = ld2u(p_sol + c[u][0]);
    pj[u][0] = q.x;
    pj[u][1] = q.y;
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (c[u][1] != c[u][0] + 1) pj[u][1] = p_sol[c[u][1]];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!lg2_on(lw[k], r0 + u)) continue;
      cu[k] += (k ? g[u].z : g[u].x) * pj[u][k];
      cv[k] += (k ? g[u].w : g[u].y) * pj[u][k];
    }
}
template <bool D16>
__global__ void __launch_bounds__(kBlock) k_precond_correct2(CoupledMatrix A, const float* __restrict__ w_in,
                                                             const float* __restrict__ binv, int jv,
                                                             const float* __restrict__ p_sol,
                                                             const float* __restrict__ dinv_uv,
                                                             float* __restrict__ z) {
  constexpr int U = CFD_CORRECT_U, U1 = CFD_CORRECT_U1;
  uint32_t i0;
  if (!row_range2(A.r0, A.r1, A.r2, A.r3, i0)) return;
  const ushort2 lg = *reinterpret_cast<const ushort2*>(A.lg + i0);
  // the row pair's own operands issued with the header (no round trip after the slots)
  const float sc = binv[jv];
  const float* wb = w_in + 3 * (size_t)i0;
  const f4u wa = ld4u(wb);
  const f2u wc = ld2u(wb + 4);
  const float2 du = *reinterpret_cast<const float2*>(dinv_uv + i0);
  const float2 ps = *reinterpret_cast<const float2*>(p_sol + i0);
  const uint32_t lw[2] = {lg.x, lg.y};
  const uint32_t maxlen = max(lw[0] & kLgUsedMask, lw[1] & kLgUsedMask);
  float cu[2] = {0.0f, 0.0f}, cv[2] = {0.0f, 0.0f};
  if (A.reg && A.ws <= U1 && __all((lw[0] & lw[1] & kLgRegular) != 0u))  // ws <= U1: the only group
    correct2_group<D16, U1, true>(A, p_sol, i0, 0, (uint32_t)A.ws - 1u, lw, cu, cv);
  else
    correct2_group<D16, U1>(A, p_sol, i0, 0, (uint32_t)A.ws - 1u, lw, cu, cv);
  for (uint32_t r0 = U1; r0 < maxlen; r0 += U) correct2_group<D16, U>(A, p_sol, i0, r0, maxlen - 1u, lw, cu, cv);
  const float wo[6] = {wa.x, wa.y, wa.z, wa.w, wc.x, wc.y};
  const float dk[2] = {du.x, du.y}, pk[2] = {ps.x, ps.y};
  float o[6];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float ru = sc * wo[3 * k], rv = sc * wo[3 * k + 1];
    const float zu = dk[k] * ru, zv = dk[k] * rv;
    o[3 * k] = zu - dk[k] * cu[k];
    o[3 * k + 1] = zv - dk[k] * cv[k];
    o[3 * k + 2] = pk[k];
  }
  float* zo = z + 3 * (size_t)i0;
  typedef float f2v __attribute__((ext_vector_type(2)));
  *reinterpret_cast<f4u*>(zo) = f4u{o[0], o[1], o[2], o[3]};
  *reinterpret_cast<f2v*>(zo + 4) = f2v{o[4], o[5]};
}

// relax_pressure (schur_precond.wgsl:52-90) on large meshes, 4 rows per thread
// over the scalar ELL image (16-bit column deltas, u8 lengths / diagonal ranks,
// the AMG row kernels' slot groups and vector gathers): the diagonal sits in
// the slots and is skipped by its rank, every other entry is summed in slot
// order -- the reference's f32 operations (omega = 1.2, the live scalar
// matrix), row for row.
template <bool D16>
__global__ void __launch_bounds__(kBlock) k_relax_pressure4(AmgLevelDev L, const uint8_t* __restrict__ drank,
                                                            const float* __restrict__ dinv_p,
                                                            const float* __restrict__ temp_p,
                                                            const float* __restrict__ src, float* dst) {
  uint32_t i0;
  if (!row_range(L.r0, L.r1, L.r2, L.r3, i0)) return;
  const uchar4 ln = *reinterpret_cast<const uchar4*>(L.len + i0);
  const uchar4 dr = *reinterpret_cast<const uchar4*>(drank + i0);
  const uint32_t maxlen = max(max(ln.x, ln.y), max(ln.z, ln.w));
  float sg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  auto step = [&](uint32_t r0, uint32_t rmax) {
    float4 v[kU];
    float xg[kU][4];
    gather_group<D16, 1, true>(L, src, i0, r0, rmax, ln, v, xg);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t r = r0 + u;
        if (r < u4(ln, k) && r != u4(dr, k)) sg[k] += f4(v[u], k) * xg[u][k];
      }
  };
  step(0, (uint32_t)max(L.w, 1) - 1u);  // peeled first group: its loads do not wait for the lengths
  for (uint32_t r0 = kU; r0 < maxlen; r0 += kU) step(r0, maxlen - 1u);
  const float4 dp = *reinterpret_cast<const float4*>(dinv_p + i0);
  const float4 tp = *reinterpret_cast<const float4*>(temp_p + i0);
  const float4 old = *reinterpret_cast<const float4*>(dst + i0);
  const float d[4] = {dp.x, dp.y, dp.z, dp.w}, b[4] = {tp.x, tp.y, tp.z, tp.w}, o[4] = {old.x, old.y, old.z, old.w};
  float y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)  // padding rows (i >= n) keep their value
    y[k] = (i0 + k < L.n) ? wmix(o[k], d[k] * (b[k] - sg[k]), 1.2f) : o[k];
  *reinterpret_cast<float4*>(dst + i0) = make_float4(y[0], y[1], y[2], y[3]);
}

}  // namespace

void launch_spmv(const CoupledMatrix& A, const float* x, float* y, hipStream_t s, const float* b, bool nt) {
  if (A.r1 <= A.r0 && A.r3 <= A.r2) return;
  const unsigned nb = rows2x_grid(A.r0, A.r1, A.r2, A.r3);
  auto fn = A.use16 ? (nt ? k_spmv2<true, true> : k_spmv2<true, false>)
                    : (nt ? k_spmv2<false, true> : k_spmv2<false, false>);
  hipLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, A, x, y, b);
}
void launch_precond_predict(const CoupledMatrix& A, const float* w_in, const float* binv, int j,
                            const float* dinv_uv, const float* dinv_p, float* temp_p, float* p_sol,
                            float* p_prev, hipStream_t s, bool nt) {
  if (A.r1 <= A.r0 && A.r3 <= A.r2) return;
  const unsigned nb = rows2x_grid(A.r0, A.r1, A.r2, A.r3);
  auto fn = A.use16 ? (nt ? k_precond_predict2<true, true> : k_precond_predict2<true, false>)
                    : (nt ? k_precond_predict2<false, true> : k_precond_predict2<false, false>);
  hipLaunchKernelGGL(fn, dim3(nb), dim3(kBlock), 0, s, A, w_in, binv, j, dinv_uv, dinv_p, temp_p, p_sol, p_prev);
}
void launch_relax_pressure4(const AmgLevelDev& L, const uint8_t* drank, const float* dinv_p, const float* temp_p,
                            const float* src, float* dst, hipStream_t s) {
  if (L.r1 <= L.r0 && L.r3 <= L.r2) return;
  const unsigned nb = rows2_grid(L.r0, L.r1, L.r2, L.r3);
  if (L.use16)
    hipLaunchKernelGGL(k_relax_pressure4<true>, dim3(nb), dim3(kBlock), 0, s, L, drank, dinv_p, temp_p, src, dst);
  else
    hipLaunchKernelGGL(k_relax_pressure4<false>, dim3(nb), dim3(kBlock), 0, s, L, drank, dinv_p, temp_p, src, dst);
}
bool launch_relax_pressure_fused(uint32_t N, uint32_t ld, uint32_t ws, const int32_t* col, const uint32_t* len,
                                 const float* sval, const float* dinv_p, const float* temp_p, float* p_sol,
                                 float* temp, uint32_t iters, hipStream_t s) {
  if (N == 0 || N > kRelaxFusedMaxRows || iters == 0) return false;
  const size_t lds = 2 * ((size_t)kRelaxFusedMaxRows + 1) * sizeof(float);  // 64 KiB
  const dim3 g(1), b(kRelaxThreads);
  // ws = widest row incl. the diagonal: at most ws - 1 off-diagonal entries per row
#define CFD_RELAX_FUSED_CASE(RPT, OD)                                                                         \
  if (N <= (uint32_t)(RPT) * kRelaxThreads && ws <= (uint32_t)(OD) + 1u) {                                    \
    hipLaunchKernelGGL((k_relax_pressure_fused<RPT, OD>), g, b, lds, s, N, ld, col, len, sval, dinv_p, temp_p, \
                       p_sol, temp, iters);                                                                   \
    return true;                                                                                              \
  }
  CFD_RELAX_FUSED_CASE(1, 15)  // register budget at 1024 threads: 128 VGPRs (the 8 x 4 case spills 16)
  CFD_RELAX_FUSED_CASE(2, 15)
  CFD_RELAX_FUSED_CASE(4, 9)
  CFD_RELAX_FUSED_CASE(8, 4)
#undef CFD_RELAX_FUSED_CASE
  return false;
}
void launch_precond_correct(const CoupledMatrix& A, const float* w_in, const float* binv, int j,
                            const float* p_sol, const float* dinv_uv, float* z, hipStream_t s) {
  if (A.r1 <= A.r0 && A.r3 <= A.r2) return;
  const unsigned nb = rows2x_grid(A.r0, A.r1, A.r2, A.r3);
  if (A.use16)
    hipLaunchKernelGGL(k_precond_correct2<true>, dim3(nb), dim3(kBlock), 0, s, A, w_in, binv, j, p_sol, dinv_uv, z);
  else
    hipLaunchKernelGGL(k_precond_correct2<false>, dim3(nb), dim3(kBlock), 0, s, A, w_in, binv, j, p_sol, dinv_uv, z);
}

}  // namespace cfd2
