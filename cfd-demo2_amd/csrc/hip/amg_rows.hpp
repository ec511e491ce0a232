// Row machinery of the AMG kernels (amg.hip), shared with k_relax_pressure4
// (coupled_rows.hip) and the tail kernels (amg_tail.hip).
#pragma once
#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

// Gathers of the row kernels.  Unused ELL slots and padding rows hold the
// row's own (valid) index, so a gather can be issued unconditionally
// (ALWAYS): no branch per load; the value of an unused slot is never consumed
// (every accumulation skips r >= len), so results are unchanged.  Same-box
// A/B (round 1, C2): k_amg_smooth 84 -> 81 us; k_amg_residual keeps the
// predicated form on its MODE 0 levels.
template <bool ALWAYS = false>
__device__ __forceinline__ float gat(bool on, const float* p) {
  if constexpr (ALWAYS) {
    (void)on;
    return *p;
  } else {
    return on ? *p : 0.0f;
  }
}

// Vector gathers: the columns of one slot for consecutive rows are, for
// every interior row of a face stencil, consecutive cells (c, c+1, ...): one
// 16-byte load (dword-aligned: gfx950 global loads need only 4-byte alignment
// for multi-dword accesses) fetches them all, and only threads whose slot is
// not consecutive (boundary / cut cells) issue the per-row loads.  Cuts the
// gather instructions per wave ~4x for scalar vectors (the row kernels are
// VMEM-issue bound: SQ_WAIT_INST_ANY ~0.5-0.7 of wave cycles,
// tools/gpu_sq.sh; round 1: level-0 smoother 84 -> 78 us, Schur predict
// 198 -> 185, correct 166 -> 159).  Every vector read this way has >= 64
// floats of padding past its last (ghost) entry.
__device__ __forceinline__ bool consec4(const int c[4]) {
  return c[1] == c[0] + 1 && c[2] == c[0] + 2 && c[3] == c[0] + 3;
}

// Each thread owns 4 consecutive rows: b, x, de and every ELL slot are one
// 16-byte load per thread (coalesced 1 KiB per wavefront), column deltas are
// 8 bytes per slot, lengths 4 bytes; only the x gathers are scalar.
template <bool D16, bool NT = false>
__device__ __forceinline__ void load_cols4(const AmgLevelDev& L, size_t off, uint32_t i0,
                                           int c[4]) {
  if constexpr (D16) {
    const short4 d = ldv<NT, short4>(L.col16 + off);
    c[0] = (int)i0 + (int)d.x;
    c[1] = (int)i0 + 1 + (int)d.y;
    c[2] = (int)i0 + 2 + (int)d.z;
    c[3] = (int)i0 + 3 + (int)d.w;
  } else {
    const int4 q = ldv<NT, int4>(L.col32 + off);
    c[0] = q.x;
    c[1] = q.y;
    c[2] = q.z;
    c[3] = q.w;
  }
}

// Slots are processed in groups of kU with every load of the group issued
// before the first use (val/col, then the x gathers): ~kU x more memory-level
// parallelism per wave than a slot-at-a-time loop.  Accumulation order per
// row is unchanged (slot order).  kU = 2 since round 3: same-box A/B over
// kU = 1..4 (profiles/r03/ab_amg_u_c1.txt, _c2.txt) C1 42.90 -> 42.25 ms,
// C2 260.8 -> 259.5 ms/step; the 5 M-row level 1 (7 slots) gains most
// (residual 57.3 -> 51.3 us), level 0 (5 slots) is flat.
#ifndef CFD_AMG_U
#define CFD_AMG_U 2
#endif
constexpr int kU = CFD_AMG_U;

// MODE 1 (level 0 of a quad mesh, small latency-bound levels): slot loads
// unconditional, clamped to rmax, the first group peeled so its loads do not
// wait for the row lengths, gathers unconditional (vector gathers).  MODE 0
// (the big coarse levels, whose row lengths vary): every slot load predicated
// on the thread's longest row (avoids reading the padding of short rows);
// peeled loads with predicated gathers were slower there (A/B level 1: 62
// vs 57 us).
typedef int i4u __attribute__((ext_vector_type(4), aligned(4)));

// The prolongation prolongate_op (amg.wgsl:56-75) of a fine row f, applied to
// its value as it is read: x'[f] = x[f] + (0 + 1 * xc[agg[f]]) -- the two f32
// roundings of k_amg_prolong (0 + v turns -0 into +0, the add follows).
__device__ __forceinline__ float prolonged(float xf, float xcv) { return xf + (0.0f + 1.0f * xcv); }

// PRO: every gathered x value is the prolonged one (k_amg_smooth<..., true>):
// agg is gathered with the same columns as x (a 16-byte load where x is), then
// the coarse values -- one more dependent round trip instead of a launch.
template <bool D16, int MODE, bool ALWAYS = false, bool PRO = false, bool NT = false>
__device__ __forceinline__ void gather_group(const AmgLevelDev& L, const float* __restrict__ x,
                                             uint32_t i0, uint32_t r0, uint32_t rmax, const uchar4 ln,
                                             float4 v[kU], float xg[kU][4],
                                             const float* __restrict__ xc = nullptr) {
  int c[kU][4];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    if (MODE != 0 || r0 + u <= rmax) {
      const size_t off = (size_t)min(r0 + u, rmax) * L.stride + i0;
      v[u] = ldv<NT, float4>(L.val + off);
      load_cols4<D16, NT>(L, off, i0, c[u]);
    } else {
      v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int k = 0; k < 4; ++k) c[u][k] = (int)i0 + k;
    }
  }
  [[maybe_unused]] int ag[kU][4];
  if constexpr (ALWAYS && MODE == 1) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const f4u q = ld4u(x + c[u][0]);
      xg[u][0] = q.x;
      xg[u][1] = q.y;
      xg[u][2] = q.z;
      xg[u][3] = q.w;
      if constexpr (PRO) {
        const i4u a = *reinterpret_cast<const i4u*>(L.agg + c[u][0]);
        ag[u][0] = a.x;
        ag[u][1] = a.y;
        ag[u][2] = a.z;
        ag[u][3] = a.w;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (!consec4(c[u])) {
#pragma unroll
        for (int k = 1; k < 4; ++k) {
          xg[u][k] = x[c[u][k]];
          if constexpr (PRO) ag[u][k] = (int)L.agg[c[u][k]];
        }
      }
  } else {
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xg[u][k] = gat<ALWAYS && MODE == 1>(r0 + u < u4(ln, k), x + c[u][k]);
        // unused slots hold the row's own (valid) column: agg of a real or padding row
        if constexpr (PRO) ag[u][k] = (int)L.agg[c[u][k]];
      }
  }
  if constexpr (PRO) {
    float cv[kU][4];
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) cv[u][k] = xc[ag[u][k]];
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) xg[u][k] = prolonged(xg[u][k], cv[u][k]);
  }
}

}  // namespace cfd2
