// Device helpers shared by the gfx950 (MI355X / CDNA4) kernels of the coupled
// FV step; included by the .hip files of this directory only.
//
// Every kernel is HBM-bandwidth bound (<= 0.25 flop/B): face sweeps, SpMV on
// compressed 3x3 blocks, BLAS-1 with wavefront reductions, Jacobi smoothing,
// restriction and prolongation.  No MFMA: nothing here is a dense contraction.
// Arithmetic follows the reference WGSL operation-for-operation (file:line in
// each kernel) and is compiled with -ffp-contract=off, so results are
// bit-identical to the CPU oracle; reductions follow the canonical order of
// kernels.hpp (256 threads x 4 cells per chunk, halving tree).
#pragma once
#include <hip/hip_runtime.h>

namespace cfd2 {

constexpr int kBlock = 256;

__device__ __forceinline__ float wsmoothstep(float lo, float hi, float x) {
  const float t = fminf(fmaxf((x - lo) / (hi - lo), 0.0f), 1.0f);
  return t * t * (3.0f - 2.0f * t);
}
__device__ __forceinline__ float wmix(float a, float b, float t) { return a * (1.0f - t) + b * t; }
__device__ __forceinline__ float safe_inverse(float v) {
  return fabsf(v) > 1e-14f ? 1.0f / v : 0.0f;
}

// A fixed-value wall slot's coefficient of a passive scalar: the diffusive part
// alone (a wall carries no flux), dist_e the distance the momentum wall
// diffusion uses.  Shared by the scalar assembly, its wall-flux sum (scalar.hip)
// and the per-face surface channels (surface.hip).
__device__ __forceinline__ float scalar_wall_coef(float rd, float area, float dist_e) { return rd * area / dist_e; }

// The weighted incremental (West / Welford) update of one quantity, f64, one
// rounding per operation (include/cfd2_amd.h "Arithmetic of the time
// statistics"): w the sample's weight, r = w / (W + w) from the host.
// mean_update: d against the old mean, e against the new one; m2_update: one M
// plane's term of the pair (q of its first quantity, e of its second).
// Shared by the per-cell time statistics (timestats.hip) and the per-face
// surface statistics (surface.hip).
struct Dev {
  double d, e;
};
__device__ __forceinline__ Dev mean_update(double x, double r, double& m) {
  Dev q;
  q.d = x - m;
  m = m + r * q.d;
  q.e = x - m;
  return q;
}
__device__ __forceinline__ void m2_update(double w, const Dev& q, double e, double& M) { M += (w * q.d) * e; }

// Loads of a kernel's once-read streams (matrix slots, row headers, the rows'
// own operands) with the nontemporal policy (NT: global_load ... nt) or the
// default one.  NT is chosen per launch for the kernels that are the LAST
// readers of their matrix before it is evicted anyway, so its lines do not
// displace, in the 256 MB Infinity Cache, the vectors the next kernels read
// (Solver::nt_mask).  Same bits either way.
template <bool NT, class V>
__device__ __forceinline__ V ldx(const V* p) {
  if constexpr (!NT) {
    return *p;
  } else {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    // f4u / f2u sources are only 4-byte aligned: their loads keep that
    // alignment instead of the vector types' natural 16 / 8 bytes
    typedef unsigned int u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
    typedef unsigned int u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
    V r;
    if constexpr (sizeof(V) == 16 && alignof(V) >= 16) {
      const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
      __builtin_memcpy(&r, &t, 16);
    } else if constexpr (sizeof(V) == 16) {
      const u32x4a4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4a4*>(p));
      __builtin_memcpy(&r, &t, 16);
    } else if constexpr (sizeof(V) == 8 && alignof(V) >= 8) {
      const u32x2 t = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
      __builtin_memcpy(&r, &t, 8);
    } else if constexpr (sizeof(V) == 8) {
      const u32x2a4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x2a4*>(p));
      __builtin_memcpy(&r, &t, 8);
    } else if constexpr (sizeof(V) == 4) {
      const uint32_t t = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
      __builtin_memcpy(&r, &t, 4);
    } else if constexpr (sizeof(V) == 2) {
      const uint16_t t = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
      __builtin_memcpy(&r, &t, 2);
    } else {
      static_assert(sizeof(V) == 1, "ldx: 1, 2, 4, 8 or 16 bytes");
      const uint8_t t = __builtin_nontemporal_load(reinterpret_cast<const uint8_t*>(p));
      __builtin_memcpy(&r, &t, 1);
    }
    return r;
  }
}
// typed views for ldx of an address inside an array of another element type
template <bool NT, class V, class T>
__device__ __forceinline__ V ldv(const T* p) {
  return ldx<NT>(reinterpret_cast<const V*>(p));
}

__device__ __forceinline__ float f4(const float4& v, int k) {
  return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}
__device__ __forceinline__ uint32_t u4(const uchar4& v, int k) {
  return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}
// 4-byte-aligned vector views (gfx950 global loads need only dword alignment
// for multi-dword accesses)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ f2u ld2u(const float* p) { return *reinterpret_cast<const f2u*>(p); }
__device__ __forceinline__ f4u ld4u(const float* p) { return *reinterpret_cast<const f4u*>(p); }

inline unsigned grid_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// XCD-aware block -> tile remap (cdna_hip_programming.md T1): the dispatcher
// deals blocks round-robin over the 8 XCDs; remapping gives XCD k a contiguous
// range of rows, so the i +- n_y neighbour gathers of a structured-ish cut-cell
// mesh hit that XCD's L2.  Bijective for any grid size; a speed choice only.
// REV: each XCD walks its range from the top down.  Blocks are dispatched in
// blockIdx order, so a kernel launched right after a forward kernel over the
// same data starts on the rows whose lines that kernel touched last, which may
// still sit in the memory-side Infinity Cache (MALL, 256 MB, shared by all
// XCDs).  Order only: every row's arithmetic is unchanged.
template <bool REV = false>
__device__ __forceinline__ uint32_t xcd_block() {
  const uint32_t b = blockIdx.x, nb = gridDim.x;
  const uint32_t xcd = b & 7u, q = nb >> 3, r = nb & 7u;
  const uint32_t base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  if constexpr (REV) return base + ((xcd < r) ? q : q - 1u) - (b >> 3);
  return base + (b >> 3);
}
template <bool REV = false>
__device__ __forceinline__ uint32_t row_id() { return xcd_block<REV>() * kBlock + threadIdx.x; }

// Kernels that run top-down (xcd_block<true>) to reuse the Infinity Cache lines
// of the kernel before them (build-time tunables, tools/ab_variants.py).  Same-box
// A/B at C2 (profiles/r01/ab_reverse_order.txt): k_amg_residual, which follows
// the pre-smoother over the same level matrix, 83.1 -> 67.4 us at level 0 when
// the two sweep in opposite directions; k_spmv, which follows k_precond_correct
// over the same cval_g / column slots, 233.5 -> 223.1 us; 278.9 -> 273.5
// ms/step.  Round 3: the smoother top-down and the residual (and the fused
// residual + restriction) bottom-up instead -- the same alternation, and now
// each smoother also runs against the bottom-up kernel before it (the Schur
// prediction writing its b and x, the prolongation): level-0 smoother 77.7 ->
// 74.7 us, C2 -1.0 / -1.25 ms/step in two same-box pairs
// (profiles/r03/ab_rev_schur_early_c2.txt, ab_early_operands_c2.txt).  The CGS
// update after the dots gains nothing (its nontemporal basis reads do not stay
// in the MALL, and temporal ones cost 20 %), so the CGS kernels keep one direction.
constexpr bool kRevSpmv = true;       // k_spmv2: top-down, after the bottom-up Schur correction
constexpr bool kRevResidual = false;  // k_amg_residual / k_amg_resrestrict: bottom-up
constexpr bool kRevSmooth = true;     // k_amg_smooth: top-down

// First row of this thread's 4 in a launch over [r0, r1) and [r2, r3) (the
// second range lets a distributed rank process both boundary strips of a
// halo'd kernel in one launch); false: no rows for this thread.
template <bool REV = false>
__device__ __forceinline__ bool row_range(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t& i0) {
  const uint32_t t = row_id<REV>(), na = (r1 - r0 + 3) / 4;
  if (t < na) {
    i0 = r0 + 4 * t;
    return i0 < r1;
  }
  i0 = r2 + 4 * (t - na);
  return i0 < r3;
}
inline unsigned rows2_grid(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
  const size_t t = (size_t)(r1 - r0 + 3) / 4 + (r3 > r2 ? (size_t)(r3 - r2 + 3) / 4 : 0);
  return (unsigned)((t + 255) / 256);
}

}  // namespace cfd2
