// Passive scalar transport (kernels.hpp "scalar.hip"): the face-slot assembly
// of one field's implicit-Euler upwind system from the mass fluxes k_prepare
// left in flux_s (and, for a field on scheme 1, the gradient pass and the
// limited right-hand side), one Jacobi sweep over its slot-major ELL image, and
// the read-only field statistics.  Nothing the step reads is written.
//
// The pieces the kernels share, each written once:
//   slots4        four slots of a cell from one slot-major array, the loads in
//                 flight together (the gradient, the limited assembly, the row)
//   scalar_coef   one slot's coefficient (both assemblies: the same bits)
//   wall_slot     whether a boundary slot is a selected wall slot of ScalarBC
//                 (the boundary-condition forms of the assemblies, the gradient
//                 and the wall-flux sums)
//   scalar_row    the Jacobi row sum of kernels.hpp ScalarSystem (the sweep
//                 and the BiCGStab operator)
//   reduce_dev.hpp: sum_accumulate / sum_store (a block's f64 sums), wave_max /
//                 block_of4_max (its maxima), k_block_fold (the maxima of all
//                 blocks)
// The sweep and the pointwise kernels run thread per cell (row_id); the kernels
// that sum run over blocks of kRedBlockCells cells, chunk by chunk.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// Slots k0 .. k0 + 3 of cell i from a slot-major array of row stride ld: four
// coalesced wavefront loads; a slot >= nf is `off` and loads nothing.
template <bool NT = false, class T>
__device__ __forceinline__ void slots4(const T* p, uint32_t ld, uint32_t i, uint32_t k0, uint32_t nf, T off,
                                       T (&v)[4]) {
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) v[j] = k0 + j < nf ? ldx<NT>(p + ((size_t)(k0 + j) * ld + i)) : off;
}

// One slot's coefficient: diff = (density * D) * area / dist_e, cin = max(-F, 0),
// c = cin + diff, in this order (tests/scalar_ref.py restates it)
__device__ __forceinline__ float scalar_coef(float rd, float F, float area, float dist_e) {
  const float diff = rd * area / dist_e;
  const float cin = F < 0.0f ? -F : 0.0f;
  return cin + diff;
}
// scalar_wall_coef, a fixed-value wall slot's coefficient: device_util.hpp
// (surface.hip evaluates the same term per face)
// Boundary slot k of type bt is a selected wall slot of the cell's image word
// (kernels.hpp ScalarBC: bits 0..30; the host refuses a selected face beyond)
__device__ __forceinline__ bool wall_slot(uint32_t sel, uint32_t k, uint32_t bt) {
  return bt == 3u && k < 31u && ((sel >> k) & 1u) != 0u;
}
constexpr uint32_t kSelWalls = 0x7FFFFFFFu;  // the wall-slot bits of an image word; bit 31: a source cell

// Thread per cell (row_id: blocks remapped per XCD), every slot load one
// coalesced wavefront access.  BC: the form with wall conditions and sources
// (kernels.hpp ScalarBC): one more coalesced load, the cell's image word, and a
// bit test on wall slots only.
template <bool BC>
__device__ __forceinline__ void scalar_assemble(const ScalarAssembleArgs& a, const ScalarBC& bc) {
  const uint32_t i = row_id();
  const uint32_t N = a.N;
  if (i >= N) return;
  const FaceSlots fs = a.fs;
  const float vol = a.vol[i];
  const float a_t = vol * a.density / a.dt;
  const float rd = a.density * a.diffusivity;
  float diag = a_t;
  float b = a_t * a.phi_old[i];
  uint32_t sel = 0;
  if constexpr (BC) sel = bc.sel[i];
  const uint32_t nf = fs.nface[i];
  for (uint32_t k = 0; k < nf; ++k) {
    const size_t e = (size_t)k * N + i;
    const uint32_t bt = fs.meta[e] & kMetaBtypeMask;
    const bool internal = fs.other[e] != kNoCell;
    float c = 0.0f;  // wall: zero flux; outlet: zero gradient, flux >= 0 by construction
    if (internal || bt == 1u) c = scalar_coef(rd, a.flux_s[e], fs.area[e], fs.dist_e[e]);  // flux_s: out of this cell
    if constexpr (BC) {
      if (!internal && wall_slot(sel, k, bt)) {
        if (bc.kind == 1) {
          c = scalar_wall_coef(rd, fs.area[e], fs.dist_e[e]);
          b += c * bc.value;
        } else {
          b += bc.value * fs.area[e];
        }
      }
    }
    a.coef[(size_t)k * a.ld + i] = c;
    diag += c;
    if (!internal && bt == 1u) b += c * a.inlet_value;
  }
  if constexpr (BC) {
    if (sel >> 31) b += vol * bc.rate;
  }
  a.diag[i] = diag;
  a.b[i] = b;
}
__global__ void __launch_bounds__(kBlock) k_scalar_assemble(ScalarAssembleArgs a) {
  scalar_assemble<false>(a, ScalarBC{});
}
__global__ void __launch_bounds__(kBlock) k_scalar_assemble_bc(ScalarAssembleArgs a, ScalarBC bc) {
  scalar_assemble<true>(a, bc);
}

// ---- scheme 1, "limited linear" (kernels.hpp ScalarGradArgs / ScalarLimitedArgs) ----
// The Green-Gauss gradient of phi_old, thread per cell: the face values of
// prepare_cell's vfu branch (flux.hip), the slots four at a time (slots4, then
// the four gathers in flight together), the sums in slot order; one 8-byte store.
// BC (a field with fixed-value walls): the face value of a selected wall slot
// is the wall's value.
template <bool BC>
__device__ __forceinline__ void scalar_grad(const ScalarGradArgs& a, const ScalarBC& bc) {
  const uint32_t i = row_id();
  const uint32_t N = a.N;
  if (i >= N) return;
  const FaceSlots fs = a.fs;
  const float pc = a.phi_old[i];
  const float vol = a.vol[i];
  float gx = 0.0f, gy = 0.0f;
  uint32_t sel = 0;
  if constexpr (BC) sel = bc.sel[i];
  const uint32_t nf = fs.nface[i];
  for (uint32_t k0 = 0; k0 < nf; k0 += 4) {
    int32_t o[4];
    uint32_t mt[4];
    float ar[4], nx[4], ny[4], lam[4], po[4];
    slots4(fs.other, N, i, k0, nf, kNoCell, o);
    slots4(fs.meta, N, i, k0, nf, 0u, mt);
    slots4(fs.area, N, i, k0, nf, 0.0f, ar);
    slots4(fs.nx, N, i, k0, nf, 0.0f, nx);
    slots4(fs.ny, N, i, k0, nf, 0.0f, ny);
    slots4(fs.lam_s, N, i, k0, nf, 0.0f, lam);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) po[j] = o[j] != kNoCell ? a.phi_old[o[j]] : 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (k0 + j >= nf) continue;  // an unused slot adds nothing, not even +0
      float vf;
      if (o[j] != kNoCell)
        vf = (mt[j] & kMetaDegen) == 0 ? lam[j] * pc + (1.0f - lam[j]) * po[j] : 0.5f * (pc + po[j]);
      else
        vf = (mt[j] & kMetaBtypeMask) == 1u ? a.inlet_value : pc;
      if constexpr (BC) {
        if (o[j] == kNoCell && wall_slot(sel, k0 + j, mt[j] & kMetaBtypeMask)) vf = bc.value;
      }
      gx += vf * nx[j] * ar[j];
      gy += vf * ny[j] * ar[j];
    }
  }
  a.g[i] = make_float2(gx / vol, gy / vol);
}
__global__ void __launch_bounds__(kBlock) k_scalar_grad(ScalarGradArgs a) { scalar_grad<false>(a, ScalarBC{}); }
__global__ void __launch_bounds__(kBlock) k_scalar_grad_bc(ScalarGradArgs a, ScalarBC bc) {
  scalar_grad<true>(a, bc);
}

// k_scalar_assemble with the limited right-hand side: the same coef and diag;
// b_i = clamp(a_t phi_old_i - corr_i) + the inlet terms.  Per internal slot one
// gather of phi_old[o] and, where the neighbour is the upwind cell, one 8-byte
// gather of g[o].  The inlet products wait for the clamp: their slots are
// remembered as a bit mask and their coefficients formed again afterwards
// (the same expression, the same bits).  The block's clamped cells: a ballot
// and a population count per wavefront, one atomic add per block.
// BC (kernels.hpp ScalarBC): the selected wall slots are the image word's low
// 31 bits, so they join the inlet mask's pass after the clamp -- one pass in
// ascending slot order over both -- without a per-slot array; a fixed-value
// slot also widens the clamp's range by its value.  The source comes last.
template <bool BC>
__device__ __forceinline__ void scalar_assemble_limited(const ScalarLimitedArgs& q, const ScalarBC& bc) {
  __shared__ uint32_t lcnt[kBlock / 64];
  const ScalarAssembleArgs& a = q.a;
  const uint32_t i = row_id();
  const uint32_t N = a.N;
  bool clamped = false;
  if (i < N) {
    const FaceSlots fs = a.fs;
    const float a_t = a.vol[i] * a.density / a.dt;
    const float rd = a.density * a.diffusivity;
    const float pc = a.phi_old[i];
    const float2 gc = q.g[i];
    float diag = a_t, corr = 0.0f, mn = pc, mx = pc;
    uint32_t inlets = 0;  // bit k: slot k is an inlet slot (the host refuses wf > 32)
    uint32_t sel = 0;
    if constexpr (BC) sel = bc.sel[i];
    const uint32_t nf = fs.nface[i];
    for (uint32_t k0 = 0; k0 < nf; k0 += 4) {
      int32_t o[4];
      uint32_t mt[4];
      float F[4], ar[4], de[4], dx[4], dy[4], po[4];
      float2 go[4];
      slots4(fs.other, N, i, k0, nf, kNoCell, o);
      slots4(fs.meta, N, i, k0, nf, 0u, mt);
      slots4(a.flux_s, N, i, k0, nf, 0.0f, F);
      slots4(fs.area, N, i, k0, nf, 0.0f, ar);
      slots4(fs.dist_e, N, i, k0, nf, 1.0f, de);
      slots4(fs.dvx, N, i, k0, nf, 0.0f, dx);
      slots4(fs.dvy, N, i, k0, nf, 0.0f, dy);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const bool in = o[j] != kNoCell;
        po[j] = in ? a.phi_old[o[j]] : 0.0f;
        go[j] = in && F[j] < 0.0f ? q.g[o[j]] : gc;
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = k0 + j;
        if (k >= nf) continue;
        const uint32_t bt = mt[j] & kMetaBtypeMask;
        const bool internal = o[j] != kNoCell;
        float c = internal || bt == 1u ? scalar_coef(rd, F[j], ar[j], de[j]) : 0.0f;
        if constexpr (BC) {
          if (!internal && bc.kind == 1 && wall_slot(sel, k, bt)) {
            c = scalar_wall_coef(rd, ar[j], de[j]);
            mn = bc.value < mn ? bc.value : mn;
            mx = bc.value > mx ? bc.value : mx;
          }
        }
        a.coef[(size_t)k * a.ld + i] = c;
        diag += c;
        if (internal) {
          mn = po[j] < mn ? po[j] : mn;
          mx = po[j] > mx ? po[j] : mx;
          if (F[j] > 0.0f || F[j] < 0.0f) {
            const bool own = F[j] > 0.0f;  // this cell is the upwind one
            const float d = own ? po[j] - pc : pc - po[j];
            const float2 gu = own ? gc : go[j];
            const float dot = gu.x * dx[j] + gu.y * dy[j];
            const float gd = own ? dot : -dot;
            float h = 0.0f;
            if (d != 0.0f) {
              const float r = (2.0f * gd) / d - 1.0f;
              const float psi = r > 0.0f ? 2.0f / (1.0f + 1.0f / r) : 0.0f;
              h = (0.5f * psi) * d;
            }
            corr += F[j] * h;
          }
        } else if (bt == 1u) {
          mn = a.inlet_value < mn ? a.inlet_value : mn;
          mx = a.inlet_value > mx ? a.inlet_value : mx;
          inlets |= 1u << k;
        }
      }
    }
    a.diag[i] = diag;
    float t = a_t * pc - corr;
    const float lo = a_t * mn, hi = a_t * mx;
    clamped = t < lo || t > hi;
    t = t < lo ? lo : (t > hi ? hi : t);
    float b = t;
    if constexpr (!BC) {
      while (inlets) {
        const uint32_t k = (uint32_t)__ffs((int)inlets) - 1u;
        inlets &= inlets - 1u;
        const size_t e = (size_t)k * N + i;
        b += scalar_coef(rd, a.flux_s[e], fs.area[e], fs.dist_e[e]) * a.inlet_value;
      }
    } else {
      uint32_t late = inlets | (sel & kSelWalls);  // an image bit is set on wall slots only
      while (late) {
        const uint32_t k = (uint32_t)__ffs((int)late) - 1u;
        late &= late - 1u;
        const size_t e = (size_t)k * N + i;
        if ((inlets >> k) & 1u)
          b += scalar_coef(rd, a.flux_s[e], fs.area[e], fs.dist_e[e]) * a.inlet_value;
        else if (bc.kind == 1)
          b += scalar_wall_coef(rd, fs.area[e], fs.dist_e[e]) * bc.value;
        else
          b += bc.value * fs.area[e];
      }
      if (sel >> 31) b += a.vol[i] * bc.rate;
    }
    a.b[i] = b;
  }
  const unsigned long long votes = __ballot(clamped);
  if ((threadIdx.x & 63) == 0) lcnt[threadIdx.x >> 6] = (uint32_t)__popcll(votes);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n = (lcnt[0] + lcnt[1]) + (lcnt[2] + lcnt[3]);
    if (n) atomicAdd(q.clamped, n);
  }
}
__global__ void __launch_bounds__(kBlock) k_scalar_assemble_limited(ScalarLimitedArgs q) {
  scalar_assemble_limited<false>(q, ScalarBC{});
}
__global__ void __launch_bounds__(kBlock) k_scalar_assemble_limited_bc(ScalarLimitedArgs q, ScalarBC bc) {
  scalar_assemble_limited<true>(q, bc);
}

// The Jacobi row sum of cell i (kernels.hpp ScalarSystem) over the vector `in`,
// from sum0: the slots four at a time -- the four column and coefficient
// loads, then the four gathers, in flight together -- and the sum itself left
// to right in slot order.  NT: the matrix streams are loaded nontemporally.
template <bool NT>
__device__ __forceinline__ float scalar_row(const int32_t* other, const float* coef, uint32_t N, uint32_t ld,
                                            uint32_t nf, uint32_t i, const float* in, float s) {
  for (uint32_t k0 = 0; k0 < nf; k0 += 4) {
    int32_t o[4];
    float c[4], p[4];
    slots4<NT>(other, N, i, k0, nf, kNoCell, o);
    slots4<NT>(coef, ld, i, k0, nf, 0.0f, c);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) p[j] = o[j] != kNoCell ? in[o[j]] : 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      if (o[j] != kNoCell) s += c[j] * p[j];  // boundary slots are skipped
  }
  return s;
}

// One Jacobi sweep, thread per cell: scalar_row from b_i, a true division.
// DELTA: also the block's maximum of |phi_out - phi_in| as a bit pattern.
template <bool DELTA>
__global__ void __launch_bounds__(kBlock) k_scalar_sweep(ScalarSweepArgs a) {
  __shared__ uint32_t lmax[kBlock / 64];
  const ScalarSystem& m = a.sys;
  const uint32_t N = m.N;
  const uint32_t lb = xcd_block();
  const uint32_t i = lb * kBlock + threadIdx.x;
  uint32_t bits = 0;
  if (i < N) {
    const float b = m.b[i];
    const float dg = m.diag[i];
    const float v = scalar_row<false>(m.other, m.coef, N, m.ld, m.nface[i], i, a.phi_in, b) / dg;
    a.phi_out[i] = v;
    if constexpr (DELTA) bits = abs_bits(v - a.phi_in[i]);
  }
  if constexpr (DELTA) {
    bits = wave_max(bits);
    if (red_lane() == 0) lmax[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) a.blockmax[lb] = block_of4_max(lmax);
  }
}

// Field statistics: the integral over the shared skeleton (reduce_dev.hpp
// sum_accumulate / sum_store), the minimum and maximum as keys.
__global__ void __launch_bounds__(kBlock) k_scalar_stats(ScalarStatsArgs a) {
  __shared__ double lsum[1][4][4];  // [sum][chunk q][quarter w]
  __shared__ uint32_t lmm[2][4];
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t kmin = ~0u, kmax = 0u;
  sum_accumulate<1>(lsum, N, lb, [&](uint32_t ci, double* t) {
    const float ph = a.phi[ci];
    t[0] = (double)a.vol[ci] * (double)ph;
    if (ph == ph) {
      const uint32_t key = scalar_value_key(__float_as_uint(ph));
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
    }
  });
  kmin = wave_min(kmin);
  kmax = wave_max(kmax);
  if (lane == 0) {
    lmm[0][w] = kmin;
    lmm[1][w] = kmax;
  }
  __syncthreads();
  sum_store<1>(lsum, a.out, N, lb);
  if (threadIdx.x == 64) {
    a.blockmm[2 * (size_t)lb] = block_of4_min(lmm[0]);
    a.blockmm[2 * (size_t)lb + 1] = block_of4_max(lmm[1]);
  }
}

// The wall-flux sums (kernels.hpp ScalarWallFluxArgs) over the shared skeleton:
// a cell with a selected slot walks the set bits of its image word in
// ascending order, every other cell loads that word alone.  Read-only.
__global__ void __launch_bounds__(kBlock) k_scalar_wall_flux(ScalarWallFluxArgs a) {
  __shared__ double lsum[kWallFluxSums][4][4];  // [sum][chunk q][quarter w]
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  sum_accumulate<kWallFluxSums>(lsum, N, lb, [&](uint32_t i, double* t) {
    uint32_t walls = a.sel[i] & kSelWalls;
    if (walls) {
      const double ph = (double)a.phi[i];
      while (walls) {
        const uint32_t k = (uint32_t)__ffs((int)walls) - 1u;
        walls &= walls - 1u;
        const size_t e = (size_t)k * N + i;
        const float area = a.area[e];
        if (a.kind == 1)
          t[0] += (double)scalar_wall_coef(a.rd, area, a.dist_e[e]) * ((double)a.value - ph);
        else
          t[0] += (double)a.value * (double)area;
        t[1] += (double)area;
        t[2] += (double)area * ph;
      }
    }
  });
  __syncthreads();
  sum_store<kWallFluxSums>(lsum, a.out, N, lb);
}

// The buoyancy body force (kernels.hpp BuoyancyForceArgs), two sums over the
// shared skeleton: per cell one 4-byte load per driving field and the volume.
// Read-only.
__global__ void __launch_bounds__(kBlock) k_buoyancy_force(BuoyancyForceArgs a) {
  __shared__ double lsum[kBuoyancySums][4][4];  // [component][chunk q][quarter w]
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  const double gx = (double)a.b.gx, gy = (double)a.b.gy;
  sum_accumulate<kBuoyancySums>(lsum, N, lb, [&](uint32_t ci, double* t) {
    const double vr = (double)a.vol[ci] * (double)a.density;
#pragma unroll
    for (int f = 0; f < kMaxBuoyancyFields; ++f) {  // unrolled: every entry a fixed kernel-argument offset
      if (f < a.b.n) {
        const double m = (vr * (double)a.b.f[f].beta) * ((double)a.b.f[f].phi[ci] - (double)a.b.f[f].ref);
        t[0] = t[0] - m * gx;
        t[1] = t[1] - m * gy;
      }
    }
  });
  __syncthreads();
  sum_store<kBuoyancySums>(lsum, a.out, N, lb);
}

// ---- BiCGStab on the Jacobi-scaled system (kernels.hpp ScalarKrylovArgs) ----
// The matrix streams (columns, coefficients, diag, b) are read once per pass
// and are larger than the Infinity Cache at the sizes this solver is for: they
// are loaded nontemporally so the work vectors keep their lines.  Same bits.
#ifndef CFD_SCALAR_KRYLOV_NT
#define CFD_SCALAR_KRYLOV_NT 1
#endif
constexpr bool kKryNT = CFD_SCALAR_KRYLOV_NT != 0;
constexpr int kKryInit = 0, kKryV = 1, kKryT = 2;

// One operator pass with its dots.  kKryInit: r = rh = p = J(x) - x, <r, r>,
// the block maximum of |r|.  kKryV: v = A p, <rh, v>.  kKryT: t = A s, <t, s>,
// <t, t>.  A p = p - J0(p), J0 = scalar_row from 0 over the diagonal.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_scalar_krylov_op(ScalarKrylovArgs a) {
  constexpr int ND = MODE == kKryT ? 2 : 1;
  __shared__ double lsum[ND][4][4];  // [dot][chunk q][quarter w]
  __shared__ uint32_t lmax[kBlock / 64];
  if (MODE != kKryInit && a.state->st[kKryDone]) return;
  const ScalarSystem& m = a.sys;
  const uint32_t N = m.N;
  const uint32_t lb = xcd_block();
  const float* __restrict__ in = MODE == kKryInit ? a.x : (MODE == kKryV ? a.p : a.s);
  float* __restrict__ out = MODE == kKryInit ? a.r : (MODE == kKryV ? a.v : a.t);
  uint32_t bits = 0;
  sum_accumulate<ND>(lsum, N, lb, [&](uint32_t i, double* t) {
    const float sum0 = MODE == kKryInit ? ldx<kKryNT>(m.b + i) : 0.0f;
    const float dg = ldx<kKryNT>(m.diag + i);
    const float qd = scalar_row<kKryNT>(m.other, m.coef, N, m.ld, m.nface[i], i, in, sum0) / dg;
    const float own = in[i];
    const float res = MODE == kKryInit ? qd - own : own - qd;
    out[i] = res;
    if constexpr (MODE == kKryInit) {
      a.rh[i] = res;
      a.p[i] = res;
      t[0] = (double)res * (double)res;
      const uint32_t ab = abs_bits(res);
      bits = ab > bits ? ab : bits;
    } else if constexpr (MODE == kKryV) {
      t[0] = (double)a.rh[i] * (double)res;
    } else {
      t[0] = (double)res * (double)own;
      t[1] = (double)res * (double)res;
    }
  });
  if constexpr (MODE == kKryInit) {
    bits = wave_max(bits);
    if (red_lane() == 0) lmax[threadIdx.x >> 6] = bits;
  }
  __syncthreads();
  sum_store<ND>(lsum, a.out, N, lb);
  if constexpr (MODE == kKryInit) {
    if (threadIdx.x == 64) a.blockmax[lb] = block_of4_max(lmax);
  }
}

// s = r - alpha v
__global__ void __launch_bounds__(kBlock) k_scalar_krylov_s(ScalarKrylovArgs a) {
  if (a.state->st[kKryDone]) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.sys.N) return;
  const float alpha = a.state->co[0];
  a.s[i] = a.r[i] - alpha * a.v[i];
}

// mode 0: x = (x + alpha p) + omega s, r = s - omega t; mode 1 (<t, t> == 0):
// x = x + alpha p, r = s; mode 2: nothing.  With <rh, r> and the block maxima of |r|.
__global__ void __launch_bounds__(kBlock) k_scalar_krylov_xr(ScalarKrylovArgs a) {
  __shared__ double lsum[1][4][4];  // [dot][chunk q][quarter w]
  __shared__ uint32_t lmax[kBlock / 64];
  const uint32_t mode = a.state->st[kKryMode];
  if (mode == 2u) return;
  const uint32_t N = a.sys.N;
  const uint32_t lb = xcd_block();
  const float alpha = a.state->co[0], omega = a.state->co[1];
  uint32_t bits = 0;
  sum_accumulate<1>(lsum, N, lb, [&](uint32_t i, double* t) {
    const float si = a.s[i];
    float xn = a.x[i] + alpha * a.p[i];
    float rn = si;
    if (mode == 0u) {
      xn = xn + omega * si;
      rn = si - omega * a.t[i];
    }
    a.x[i] = xn;
    a.r[i] = rn;
    t[0] = (double)a.rh[i] * (double)rn;
    const uint32_t ab = abs_bits(rn);
    bits = ab > bits ? ab : bits;
  });
  bits = wave_max(bits);
  if (red_lane() == 0) lmax[threadIdx.x >> 6] = bits;
  __syncthreads();
  sum_store<1>(lsum, a.out, N, lb);
  if (threadIdx.x == 64) a.blockmax[lb] = block_of4_max(lmax);
}

// p = r + beta (p - omega v)
__global__ void __launch_bounds__(kBlock) k_scalar_krylov_p(ScalarKrylovArgs a) {
  if (a.state->st[kKryDone]) return;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.sys.N) return;
  const float omega = a.state->co[1], beta = a.state->co[2];
  a.p[i] = a.r[i] + beta * (a.p[i] - omega * a.v[i]);
}

template <int NT>
__device__ __forceinline__ uint32_t block_max32(const uint32_t* __restrict__ v, uint32_t nb, uint32_t* l) {
  uint32_t m = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += NT) m = v[b] > m ? v[b] : m;
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) l[threadIdx.x >> 6] = m;
  __syncthreads();
  uint32_t r = 0;
  for (uint32_t w = 0; w < NT / 64; ++w) r = l[w] > r ? l[w] : r;
  __syncthreads();
  return r;
}
__device__ __forceinline__ bool kry_bad(double v) { return v == 0.0 || !isfinite(v); }
__device__ __forceinline__ bool kry_bad(float v) { return v == 0.0f || !isfinite(v); }
__device__ __forceinline__ void kry_stop(uint32_t* st, uint32_t reason, uint32_t iter) {
  st[kKryDone] = 1u;
  st[kKryReason] = reason;
  st[kKryIter] = iter;
}

// One block finishes a stage: the totals of its dots by the segment and total
// trees, the coefficient in f64 and rounded to f32, the status words.
constexpr int kKryFinStart = 0, kKryFinAlpha = 1, kKryFinOmega = 2, kKryFinBeta = 3;
template <int STAGE>
__global__ void __launch_bounds__(kRedFinalThreads) k_scalar_krylov_fin(ScalarKrylovArgs a, uint32_t nb, uint32_t k,
                                                                        uint32_t max_iters) {
  __shared__ double la[kRedMaxSegments], lb[65];
  __shared__ uint32_t lm[kRedFinalThreads / 64];
  uint32_t* st = a.state->st;
  double* dv = a.state->dv;
  float* co = a.state->co;
  const uint32_t done = STAGE == kKryFinStart ? 0u : st[kKryDone];
  const uint32_t mode = STAGE == kKryFinBeta ? st[kKryMode] : 0u;
  __syncthreads();  // every thread has read the words thread 0 writes below
  if constexpr (STAGE == kKryFinStart) {
    const uint32_t res = block_max32<kRedFinalThreads>(a.blockmax, nb, lm);
    const double rho = red_total<double, kRedFinalThreads>(a.red, 0, la, lb);
    if (threadIdx.x == 0) {
      const bool stop = __uint_as_float(res) <= a.tol;
      st[kKryDone] = stop ? 1u : 0u;
      st[kKryReason] = stop ? 1u : 0u;
      st[kKryIter] = 0u;
      st[kKryRes] = res;
      st[kKryMode] = 2u;
      dv[0] = rho;
      dv[1] = dv[2] = 0.0;
      co[0] = co[1] = co[2] = 0.0f;
    }
  } else if constexpr (STAGE == kKryFinAlpha) {
    if (done) return;
    const double d = red_total<double, kRedFinalThreads>(a.red, 0, la, lb);
    if (threadIdx.x == 0) {
      const double rho = dv[0];
      const double alpha = rho / d;
      const float af = (float)alpha;
      if (kry_bad(rho) || kry_bad(d) || kry_bad(af)) {
        kry_stop(st, 2u, k);
        co[0] = 0.0f;
      } else {
        dv[1] = alpha;
        co[0] = af;
      }
    }
  } else if constexpr (STAGE == kKryFinOmega) {
    if (done) {
      if (threadIdx.x == 0) st[kKryMode] = 2u;
      return;
    }
    const double ts = red_total<double, kRedFinalThreads>(a.red, 0, la, lb);
    const double tt = red_total<double, kRedFinalThreads>(a.red, 1, la, lb);
    if (threadIdx.x == 0) {
      if (tt == 0.0) {
        kry_stop(st, 2u, k);
        st[kKryMode] = 1u;
        co[1] = 0.0f;
      } else {
        const double omega = ts / tt;
        const float of = (float)omega;
        if (!isfinite(tt) || kry_bad(of)) {
          kry_stop(st, 2u, k);
          st[kKryMode] = 2u;
          co[1] = 0.0f;
        } else {
          st[kKryMode] = 0u;
          dv[2] = omega;
          co[1] = of;
        }
      }
    }
  } else {
    if (mode == 2u) return;  // this iteration stopped before its x / r update
    const uint32_t res = block_max32<kRedFinalThreads>(a.blockmax, nb, lm);
    const double rho1 = red_total<double, kRedFinalThreads>(a.red, 0, la, lb);
    if (threadIdx.x == 0) {
      st[kKryRes] = res;
      if (done) return;  // mode 1: the stop is already recorded
      if (__uint_as_float(res) <= a.tol) {
        kry_stop(st, 1u, k);
        return;
      }
      if (k >= max_iters) return;  // the host records reason 3
      const double beta = (rho1 / dv[0]) * (dv[1] / dv[2]);
      const float bf = (float)beta;
      if (kry_bad(rho1) || kry_bad(bf)) {
        kry_stop(st, 2u, k + 1u);
        co[2] = 0.0f;
      } else {
        dv[0] = rho1;
        co[2] = bf;
      }
    }
  }
}

}  // namespace

void launch_scalar_krylov_start(const ScalarKrylovArgs& a, hipStream_t s) {
  const uint32_t nb = red_blocks(a.sys.N);
  if (nb) hipLaunchKernelGGL((k_scalar_krylov_op<kKryInit>), dim3(nb), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((k_scalar_krylov_fin<kKryFinStart>), dim3(1), dim3(kRedFinalThreads), 0, s, a, nb, 0u, 0u);
}

void launch_scalar_krylov_iteration(const ScalarKrylovArgs& a, uint32_t k, uint32_t max_iters, hipStream_t s) {
  const uint32_t nb = red_blocks(a.sys.N), ne = grid_for(a.sys.N);
  if (!nb) return;
  const dim3 one(1), fin(kRedFinalThreads), blk(kBlock);
  hipLaunchKernelGGL((k_scalar_krylov_op<kKryV>), dim3(nb), blk, 0, s, a);
  hipLaunchKernelGGL((k_scalar_krylov_fin<kKryFinAlpha>), one, fin, 0, s, a, nb, k, max_iters);
  hipLaunchKernelGGL(k_scalar_krylov_s, dim3(ne), blk, 0, s, a);
  hipLaunchKernelGGL((k_scalar_krylov_op<kKryT>), dim3(nb), blk, 0, s, a);
  hipLaunchKernelGGL((k_scalar_krylov_fin<kKryFinOmega>), one, fin, 0, s, a, nb, k, max_iters);
  hipLaunchKernelGGL(k_scalar_krylov_xr, dim3(nb), blk, 0, s, a);
  hipLaunchKernelGGL((k_scalar_krylov_fin<kKryFinBeta>), one, fin, 0, s, a, nb, k, max_iters);
  if (k < max_iters) hipLaunchKernelGGL(k_scalar_krylov_p, dim3(ne), blk, 0, s, a);
}

uint32_t scalar_sweep_blocks(uint32_t N) { return grid_for(N); }

void launch_scalar_assemble(const ScalarAssembleArgs& a, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_scalar_assemble, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a);
}

void launch_scalar_grad(const ScalarGradArgs& a, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_scalar_grad, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a);
}

void launch_scalar_assemble_limited(const ScalarLimitedArgs& a, hipStream_t s) {
  if (!a.a.N) return;
  hipLaunchKernelGGL(k_scalar_assemble_limited, dim3(grid_for(a.a.N)), dim3(kBlock), 0, s, a);
}

void launch_scalar_assemble_bc(const ScalarAssembleArgs& a, const ScalarBC& bc, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_scalar_assemble_bc, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, bc);
}

void launch_scalar_grad_bc(const ScalarGradArgs& a, const ScalarBC& bc, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_scalar_grad_bc, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, bc);
}

void launch_scalar_assemble_limited_bc(const ScalarLimitedArgs& a, const ScalarBC& bc, hipStream_t s) {
  if (!a.a.N) return;
  hipLaunchKernelGGL(k_scalar_assemble_limited_bc, dim3(grid_for(a.a.N)), dim3(kBlock), 0, s, a, bc);
}

void launch_scalar_wall_flux(const ScalarWallFluxArgs& a, hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_scalar_wall_flux, dim3(nb), dim3(kBlock), 0, s, a);
}

void launch_buoyancy_force(const BuoyancyForceArgs& a, hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_buoyancy_force, dim3(nb), dim3(kBlock), 0, s, a);
}

void launch_scalar_sweep(const ScalarSweepArgs& a, uint32_t* delta, hipStream_t s) {
  const uint32_t nb = scalar_sweep_blocks(a.sys.N);
  if (nb) {
    if (delta)
      hipLaunchKernelGGL((k_scalar_sweep<true>), dim3(nb), dim3(kBlock), 0, s, a);
    else
      hipLaunchKernelGGL((k_scalar_sweep<false>), dim3(nb), dim3(kBlock), 0, s, a);
  }
  if (delta) hipLaunchKernelGGL(k_block_fold<uint32_t>, dim3(1), dim3(kBlock), 0, s, a.blockmax, nb, 1u, 0u, delta);
}

void launch_scalar_stats(const ScalarStatsArgs& a, ScalarResults* res, hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_scalar_stats, dim3(nb), dim3(kBlock), 0, s, a);
  static_assert(offsetof(ScalarResults, kmax) == offsetof(ScalarResults, kmin) + 4, "the fold writes the pair");
  hipLaunchKernelGGL(k_block_fold<uint32_t>, dim3(1), dim3(kBlock), 0, s, a.blockmm, nb, 2u, 1u, &res->kmin);
}

}  // namespace cfd2
