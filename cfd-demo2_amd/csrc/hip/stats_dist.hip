// check_evolution statistics and the distributed helpers (halo pack, segment
// values, max combine).
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// ---------------------- check_evolution statistics --------------------------
// AoS view of the reference FluidState (coupled_solver.rs:504 reads the 32-byte
// records as a flat f32 array): record r = {u.x, u.y, p, d_p, gp.x, gp.y, 0, 0}.
__device__ __forceinline__ void view_pair(const StateView& v, uint32_t rec, int pair, float* a,
                                          float* b) {
  if (pair == 0) {
    const float2 u = v.u[rec];
    *a = u.x;
    *b = u.y;
  } else if (pair == 1) {
    *a = v.p[rec];
    *b = v.dp[rec];
  } else if (pair == 2) {
    const float2 gp = v.gp[rec];
    *a = gp.x;
    *b = gp.y;
  } else {
    *a = 0.0f;
    *b = 0.0f;
  }
}

// `var` + (gbase, rec0): the records the variance part reads -- the record of
// global index gbase + c is ((gbase + c) >> 2) - rec0 in `var` (on one GPU:
// var = cur, gbase = rec0 = 0; distributed: records fetched from their owners).
// Leaves per cell: evolution = the 8 squared differences added in field order
// (u.x, u.y, p, d_p, grad_p.x, grad_p.y, and the unused grad_component pair,
// which is 0 - 0), then u, v, u^2, v^2 of the (stride-bug) variance record;
// chunk partials partial[f * np + k] in the canonical tree order.
__global__ void __launch_bounds__(kBlock) k_evolution_partial(StateView cur, StateView prev,
                                                              int have_prev, uint32_t N,
                                                              StateView var, uint64_t gbase,
                                                              uint64_t rec0, uint32_t U, double* partial,
                                                              uint32_t np) {
  __shared__ double lds[5 * 4];
  const uint32_t k = red_chunk();
  const uint32_t c0 = k * kRedChunkCells + 4 * red_lane();
  double lf[5][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t c = c0 + q;
    double evo = 0.0, a_d = 0.0, b_d = 0.0;
    if (c < N) {
      if (have_prev) {
        bool first = true;
        for (int pr = 0; pr < 4; ++pr) {
          float a0, b0, a1, b1;
          view_pair(cur, c, pr, &a0, &b0);
          view_pair(prev, c, pr, &a1, &b1);
          const float da = a0 - a1, db = b0 - b1;
          const double ta = (double)(da * da), tb = (double)(db * db);
          evo = first ? ta : evo + ta;
          evo = evo + tb;
          first = false;
        }
      }
      float a, b;
      const uint64_t gi = gbase + c;
      view_pair(var, (uint32_t)((gi >> 2) - rec0), (int)(gi & 3), &a, &b);
      a_d = (double)a;
      b_d = (double)b;
    }
    lf[0][q] = evo;
    lf[1][q] = a_d;
    lf[2][q] = b_d;
    lf[3][q] = a_d * a_d;
    lf[4][q] = b_d * b_d;
  }
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const double r = wave_tree((lf[f][0] + lf[f][1]) + (lf[f][2] + lf[f][3]));
    if (red_lane() == 0) lds[4 * f + (threadIdx.x >> 6)] = r;
  }
  __syncthreads();
  const uint32_t UB = 4 / U;
  if (threadIdx.x < 5 * UB) {
    const uint32_t f = threadIdx.x / UB, u = threadIdx.x % UB, unit = blockIdx.x * UB + u;
    if ((size_t)unit * U * kRedChunkCells < N && unit < np) partial[(size_t)f * np + unit] = unit_value(lds + 4 * f, U, u);
  }
}

__global__ void __launch_bounds__(kRedFinalThreads) k_evolution_final(RedSrcD r, double* out) {
  __shared__ double la[kRedMaxSegments], lb[65];
  for (uint32_t f = 0; f < r.nvec; ++f) {
    const double t = red_total<double, kRedFinalThreads>(r, f, la, lb);
    if (threadIdx.x == 0) out[f] = t;
  }
}

// ------------------------- distributed helpers ------------------------------
// Halo pack: for every field f, stage[off_f + k*comps_f + c] = src_f[idx[k]*comps_f + c]
// (idx = owned rows the peers need, concatenated per peer, ascending global id).
__global__ void __launch_bounds__(kBlock) k_pack(PackArgs a) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= a.n) return;
  const int32_t i = a.idx[k];
  for (int f = 0; f < a.nf; ++f) {
    const PackField F = a.f[f];
    for (int c = 0; c < F.comps; ++c)
      a.stage[F.stage_off + (size_t)k * F.comps + c] = F.src[(ptrdiff_t)i * F.comps + c];
  }
}

// Distributed: this rank's segment values of nvec reductions, one wavefront
// per segment: out[v * maxseg + s] (blockIdx.y = v).
template <class T>
__global__ void __launch_bounds__(kBlock) k_seg_reduce(const T* __restrict__ part, uint32_t np, uint32_t nchunks,
                                                       uint32_t G, T* out, uint32_t maxseg) {
  const uint32_t sg = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t v = blockIdx.y;
  const uint32_t nsl = (nchunks + G - 1) / G;
  T o[1];
  seg_trees<T, 1>(part + (size_t)v * np, nchunks, G, sg, 0, nsl, o);
  if (red_lane() == 0 && sg < maxseg) out[(size_t)v * maxseg + sg] = o[0];
}

// max over ranks of the (u, p) max-diff bit patterns
__global__ void k_max_combine(const uint32_t* __restrict__ gathered, int R, uint32_t* out, uint32_t* host_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t bu = 0, bp = 0;
  for (int r = 0; r < R; ++r) {
    bu = max(bu, gathered[2 * r]);
    bp = max(bp, gathered[2 * r + 1]);
  }
  out[0] = bu;
  out[1] = bp;
  if (host_out) {
    host_out[0] = bu;
    host_out[1] = bp;
  }
}

}  // namespace

void launch_evolution_partial(StateView cur, StateView prev, int have_prev, uint32_t N, StateView var,
                              uint64_t gbase, uint64_t rec0, uint32_t U, double* partial, uint32_t np,
                              hipStream_t s) {
  if (N)
    hipLaunchKernelGGL(k_evolution_partial, dim3(red_blocks(N)), dim3(kBlock), 0, s, cur, prev, have_prev, N, var,
                       gbase, rec0, U, partial, np);
}
void launch_pack(const PackArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_pack, dim3(grid_for(a.n)), dim3(kBlock), 0, s, a);
}
template <class T>
static void seg_reduce(const T* part, uint32_t np, uint32_t nchunks, uint32_t G, int nvec, T* out, uint32_t maxseg,
                       hipStream_t s) {
  if (nvec <= 0 || maxseg == 0) return;
  const unsigned nb = (maxseg + 3) / 4;
  hipLaunchKernelGGL(k_seg_reduce<T>, dim3(nb, (unsigned)nvec), dim3(kBlock), 0, s, part, np, nchunks, G, out,
                     maxseg);
}
void launch_seg_reduce(const float* part, uint32_t np, uint32_t nchunks, uint32_t G, int nvec, float* out,
                       uint32_t maxseg, hipStream_t s) {
  seg_reduce(part, np, nchunks, G, nvec, out, maxseg, s);
}
void launch_seg_reduce_d(const double* part, uint32_t np, uint32_t nchunks, uint32_t G, int nvec, double* out,
                         uint32_t maxseg, hipStream_t s) {
  seg_reduce(part, np, nchunks, G, nvec, out, maxseg, s);
}
void launch_max_combine(const uint32_t* gathered, int R, uint32_t* out, uint32_t* host_out, hipStream_t s) {
  hipLaunchKernelGGL(k_max_combine, dim3(1), dim3(64), 0, s, gathered, R, out, host_out);
}
void launch_evolution_final(const RedSrcD& r, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_evolution_final, dim3(1), dim3(kRedFinalThreads), 0, s, r, out);
}

}  // namespace cfd2
