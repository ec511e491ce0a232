// AMG V-cycle over the small levels in one workgroup (global, LDS vectors, LDS
// vectors + matrices).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>

#include "amg_rows.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// ---- single-row helpers for the one-workgroup kernels (small levels) ----
__device__ __forceinline__ int col_at(const AmgLevelDev& L, size_t off, uint32_t i) {
  return L.use16 ? (int)i + (int)L.col16[off] : L.col32[off];
}
__device__ __forceinline__ float smooth_row(const AmgLevelDev& L, const float* x, const float* b,
                                            uint32_t i) {
  float sigma = 0.0f;
  const uint32_t len = L.len16 ? (uint32_t)L.len16[i] : (uint32_t)L.len[i];
  for (uint32_t r = 0; r < len; ++r) {
    const size_t off = (size_t)r * L.stride + i;
    sigma += L.val[off] * x[col_at(L, off, i)];
  }
  return wmix(x[i], (b[i] - sigma) / L.de[i], 0.8f);
}
__device__ __forceinline__ float residual_row(const AmgLevelDev& L, const float* x, const float* b,
                                              uint32_t i) {
  const uint32_t len = L.len16 ? (uint32_t)L.len16[i] : (uint32_t)L.len[i];
  const uint32_t dr = L.drank16 ? (uint32_t)L.drank16[i] : (uint32_t)L.drank[i];
  float ax = 0.0f;
  for (uint32_t r = 0; r <= len; ++r) {
    if (r == dr) ax += L.dv[i] * x[i];
    if (r == len) break;
    const size_t off = (size_t)r * L.stride + i;
    ax += L.val[off] * x[col_at(L, off, i)];
  }
  return b[i] - ax;
}

// One workgroup runs the V-cycle over the small levels [first, nlev): every
// phase of amg.rs:666-770 with a workgroup barrier instead of a kernel boundary.
// Each level does an even number of out-of-place sweeps, so the pre-smoother
// goes x -> xt, the post-smoother xt -> x and the coarsest solve ends in x,
// exactly the host-side ping-pong of Solver::amg_smooth.
__global__ void __launch_bounds__(1024) k_amg_tail(const AmgTailLevel* __restrict__ tail, int first,
                                                   int nlev) {
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  for (int l = first; l + 1 < nlev; ++l) {
    const AmgTailLevel T = tail[l];
    for (uint32_t i = t; i < T.L.n; i += nt) T.xt[i] = smooth_row(T.L, T.x, T.b, i);
    __syncthreads();
    for (uint32_t i = t; i < T.L.n; i += nt) T.r[i] = residual_row(T.L, T.xt, T.b, i);
    __syncthreads();
    float* cb = tail[l + 1].b;
    float* cx = tail[l + 1].x;
    for (uint32_t I = t; I < T.L.nc; I += nt) {
      float sum = 0.0f;
      for (uint32_t k = T.L.r_row[I]; k < T.L.r_row[I + 1]; ++k) sum += 1.0f * T.r[T.L.r_col[k]];
      cb[I] = sum;
      cx[I] = 0.0f;
    }
    __syncthreads();
  }
  {
    const AmgTailLevel T = tail[nlev - 1];
    for (int s = 0; s < 10; ++s) {
      const float* xin = (s & 1) ? T.xt : T.x;
      float* xout = (s & 1) ? T.x : T.xt;
      for (uint32_t i = t; i < T.L.n; i += nt) xout[i] = smooth_row(T.L, xin, T.b, i);
      __syncthreads();
    }
  }
  for (int l = nlev - 2; l >= first; --l) {
    const AmgTailLevel T = tail[l];
    const float* xc = tail[l + 1].x;
    for (uint32_t i = t; i < T.L.n; i += nt) {
      float corr = 0.0f;
      corr += 1.0f * xc[T.L.agg[i]];
      T.xt[i] += corr;
    }
    __syncthreads();
    for (uint32_t i = t; i < T.L.n; i += nt) T.x[i] = smooth_row(T.L, T.xt, T.b, i);
    __syncthreads();
  }
}

// The same V-cycle tail with every vector of the tail levels in LDS (x, xt,
// b, r per level; the matrices stay in L2): each phase is one global-latency
// round (matrix row) + LDS gathers + a barrier.  Entry: b of `first` in global
// memory, x of every tail level known zero (cleared by the restriction), so
// each pre-smoother is the elementwise zero-x sweep.  Exit: x of `first`
// written back for the host-side prolongation.
__device__ __forceinline__ uint32_t r4(uint32_t n) { return (n + 3) & ~3u; }

__global__ void __launch_bounds__(1024) k_amg_tail_lds(const AmgTailLevel* __restrict__ tail, int first,
                                                       int nlev) {
  extern __shared__ float sm[];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  auto base = [&](int l) {
    uint32_t o = 0;
    for (int k = first; k < l; ++k) o += 4 * r4(tail[k].L.n);
    return sm + o;
  };
  {
    const AmgTailLevel T = tail[first];
    float* B0 = base(first) + 2 * r4(T.L.n);
    for (uint32_t i = t; i < T.L.n; i += nt) B0[i] = T.b[i];
  }
  __syncthreads();
  for (int l = first; l + 1 < nlev; ++l) {
    const AmgLevelDev L = tail[l].L;
    const uint32_t nr = r4(L.n);
    float* X = base(l);
    float* XT = X + nr;
    float* B = XT + nr;
    float* Rr = B + nr;
    for (uint32_t i = t; i < L.n; i += nt) XT[i] = wmix(0.0f, (B[i] - 0.0f) / L.de[i], 0.8f);
    __syncthreads();
    for (uint32_t i = t; i < L.n; i += nt) Rr[i] = residual_row(L, XT, B, i);
    __syncthreads();
    float* CB = base(l + 1) + 2 * r4(tail[l + 1].L.n);
    for (uint32_t I = t; I < L.nc; I += nt) {
      float sum = 0.0f;
      for (uint32_t k = L.r_row[I]; k < L.r_row[I + 1]; ++k) sum += 1.0f * Rr[L.r_col[k]];
      CB[I] = sum;
    }
    __syncthreads();
  }
  {
    const AmgLevelDev L = tail[nlev - 1].L;
    const uint32_t nr = r4(L.n);
    float* X = base(nlev - 1);
    float* XT = X + nr;
    float* B = XT + nr;
    for (int s = 0; s < 10; ++s) {
      if (s == 0) {
        for (uint32_t i = t; i < L.n; i += nt) XT[i] = wmix(0.0f, (B[i] - 0.0f) / L.de[i], 0.8f);
      } else {
        const float* xin = (s & 1) ? XT : X;
        float* xout = (s & 1) ? X : XT;
        for (uint32_t i = t; i < L.n; i += nt) xout[i] = smooth_row(L, xin, B, i);
      }
      __syncthreads();
    }
  }
  for (int l = nlev - 2; l >= first; --l) {
    const AmgLevelDev L = tail[l].L;
    const uint32_t nr = r4(L.n);
    float* X = base(l);
    float* XT = X + nr;
    float* B = XT + nr;
    const float* XC = base(l + 1);
    for (uint32_t i = t; i < L.n; i += nt) {
      float corr = 0.0f;
      corr += 1.0f * XC[L.agg[i]];
      XT[i] += corr;
    }
    __syncthreads();
    for (uint32_t i = t; i < L.n; i += nt) X[i] = smooth_row(L, XT, B, i);
    __syncthreads();
  }
  const AmgTailLevel T = tail[first];
  const float* X0 = base(first);
  for (uint32_t i = t; i < T.L.n; i += nt) T.x[i] = X0[i];
}

// The LDS tail with every matrix of the tail levels in LDS as well (the blob
// built once by the host from the level images: off-diagonal CSR with u16
// columns, dv/de, drank, P and R).  Each phase is then LDS reads + one
// barrier instead of a global (L2) round trip per matrix slot.  Same row
// arithmetic, in the same order, as smooth_row / residual_row.
// The zero-x pre-smoother is fused with the residual, and the prolongation
// with the post-smoother (two barriers fewer per level, round 3).
__global__ void __launch_bounds__(1024) k_amg_tail_blob(const AmgTailLevel* __restrict__ tail,
                                                        const TailBlobLevel* __restrict__ desc,
                                                        const uint32_t* __restrict__ blob, uint32_t blob_words,
                                                        uint32_t vec_floats, int first, int nlev,
                                                        const float* __restrict__ b_first, uint32_t n_first) {
  extern __shared__ float sm[];
  const uint32_t t = threadIdx.x, nt = blockDim.x;
  uint32_t* bw = reinterpret_cast<uint32_t*>(sm + vec_floats);
  auto base = [&](int l) {
    uint32_t o = 0;
    for (int k = first; k < l; ++k) o += 4 * r4(desc[k].n);
    return sm + o;
  };
  {
    // every global load of the blob and of b issued before the first LDS
    // store: one memory round trip instead of one per 16 KiB pass (the blob
    // is cold in HBM after the fine levels' sweeps: C2 25.2 -> 23.9 us,
    // profiles/r03/ab_tail_occ_c2.txt).  The launch is always
    // 1024 threads; blob and b together fit in kTailLdsMax (16 B per row of
    // b's level alone), so KB / KV loads per thread cover both.
    constexpr uint32_t NT = 1024, KB = (uint32_t)((kTailLdsMax / 16 + NT - 1) / NT), KV = KB;
    // b and n of the first level as kernel arguments: no dependent load of
    // the level descriptors before the b loads
    const uint32_t n = n_first;
    const float* gb = b_first;
    uint4 v[KB];
    float bv[KV];
    // clamped, unconditional loads (guarded ones put v[] in scratch)
#pragma unroll
    for (uint32_t k = 0; k < KB; ++k)
      v[k] = *reinterpret_cast<const uint4*>(blob + min(4 * (t + k * NT), blob_words - 4));
#pragma unroll
    for (uint32_t k = 0; k < KV; ++k) bv[k] = gb[min(t + k * NT, n - 1)];
    // pin the loaded registers here so that the compiler cannot sink each
    // load into its guarded store below (load -> wait -> store per pass)
#pragma unroll
    for (uint32_t k = 0; k < KB; ++k) asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w));
#pragma unroll
    for (uint32_t k = 0; k < KV; ++k) asm volatile("" : "+v"(bv[k]));
#pragma unroll
    for (uint32_t k = 0; k < KB; ++k) {
      const uint32_t w = 4 * (t + k * NT);
      if (w < blob_words) *reinterpret_cast<uint4*>(bw + w) = v[k];
    }
    float* B0 = base(first) + 2 * r4(n);
#pragma unroll
    for (uint32_t k = 0; k < KV; ++k)
      if (t + k * NT < n) B0[t + k * NT] = bv[k];
  }
  __syncthreads();
  auto fw = [&](uint32_t off) { return reinterpret_cast<const float*>(bw + off); };
  auto hw = [&](uint32_t off) { return reinterpret_cast<const uint16_t*>(bw + off); };
  auto smooth = [&](const TailBlobLevel& D, const float* xin, const float* B, uint32_t i) {
    const uint32_t* ro = bw + D.rowoff;
    const float* val = fw(D.val);
    const uint16_t* col = hw(D.col);
    float sigma = 0.0f;
    for (uint32_t e = ro[i]; e < ro[i + 1]; ++e) sigma += val[e] * xin[col[e]];
    return wmix(xin[i], (B[i] - sigma) / fw(D.de)[i], 0.8f);
  };
  for (int l = first; l + 1 < nlev; ++l) {
    const TailBlobLevel D = desc[l];
    const uint32_t nr = r4(D.n);
    float* X = base(l);
    float* XT = X + nr;
    float* B = XT + nr;
    float* Rr = B + nr;
    const float* de = fw(D.de);
    // zero-x pre-smoother and residual in one phase: a neighbour's smoothed
    // value is recomputed from its b and diagonal (the same operations as
    // the sweep), the row's own is stored for the up-sweep
    const uint32_t* ro = bw + D.rowoff;
    const float* val = fw(D.val);
    const float* dv = fw(D.dv);
    const uint16_t* col = hw(D.col);
    const uint8_t* drank = reinterpret_cast<const uint8_t*>(bw + D.drank);
    for (uint32_t i = t; i < D.n; i += nt) {
      const float xti = wmix(0.0f, (B[i] - 0.0f) / de[i], 0.8f);
      XT[i] = xti;
      const uint32_t e0 = ro[i], len = ro[i + 1] - e0, dr = drank[i];
      float ax = 0.0f;
      for (uint32_t r = 0; r <= len; ++r) {
        if (r == dr) ax += dv[i] * xti;
        if (r == len) break;
        const uint32_t j = col[e0 + r];
        ax += val[e0 + r] * wmix(0.0f, (B[j] - 0.0f) / de[j], 0.8f);
      }
      Rr[i] = B[i] - ax;
    }
    __syncthreads();
    float* CB = base(l + 1) + 2 * r4(desc[l + 1].n);
    {
      const uint16_t* rrow = hw(D.r_row);
      const uint16_t* rcol = hw(D.r_col);
      for (uint32_t I = t; I < D.nc; I += nt) {
        float sum = 0.0f;
        for (uint32_t k = rrow[I]; k < rrow[I + 1]; ++k) sum += 1.0f * Rr[rcol[k]];
        CB[I] = sum;
      }
    }
    __syncthreads();
  }
  {
    const TailBlobLevel D = desc[nlev - 1];
    const uint32_t nr = r4(D.n);
    float* X = base(nlev - 1);
    float* XT = X + nr;
    float* B = XT + nr;
    const float* de = fw(D.de);
    if (D.maxlen == 0) {
      // coarsest level without off-diagonal entries (C1: 829 rows): every
      // sweep is row-local, so each thread runs its row's 10 sweeps in
      // registers with no barrier in between -- the operations of smooth()
      // with sigma = +0 in the same order (bit-identical; (b - 0) / d is the
      // same value in every sweep)
      for (uint32_t i = t; i < D.n; i += nt) {
        const float q = (B[i] - 0.0f) / de[i];
        float xp = wmix(0.0f, q, 0.8f), xq = xp;
        for (int s = 1; s < 10; ++s) {
          xq = xp;
          xp = wmix(xq, q, 0.8f);
        }
        XT[i] = xq;  // sweep 8 (even sweeps write XT)
        X[i] = xp;   // sweep 9
      }
      __syncthreads();
    } else {
      for (int s = 0; s < 10; ++s) {
        if (s == 0) {
          for (uint32_t i = t; i < D.n; i += nt) XT[i] = wmix(0.0f, (B[i] - 0.0f) / de[i], 0.8f);
        } else {
          const float* xin = (s & 1) ? XT : X;
          float* xout = (s & 1) ? X : XT;
          for (uint32_t i = t; i < D.n; i += nt) xout[i] = smooth(D, xin, B, i);
        }
        __syncthreads();
      }
    }
  }
  for (int l = nlev - 2; l >= first; --l) {
    const TailBlobLevel D = desc[l];
    const uint32_t nr = r4(D.n);
    float* X = base(l);
    float* XT = X + nr;
    float* B = XT + nr;
    const float* XC = base(l + 1);
    const uint16_t* agg = hw(D.agg);
    // prolongation and post-smoother in one phase: every value the sweep
    // reads is prolonged as it is read (k_amg_smooth<..., PRO>'s rule)
    const uint32_t* ro = bw + D.rowoff;
    const float* val = fw(D.val);
    const uint16_t* col = hw(D.col);
    const float* de = fw(D.de);
    for (uint32_t i = t; i < D.n; i += nt) {
      float sigma = 0.0f;
      for (uint32_t e = ro[i]; e < ro[i + 1]; ++e) {
        const uint32_t j = col[e];
        sigma += val[e] * prolonged(XT[j], XC[agg[j]]);
      }
      X[i] = wmix(prolonged(XT[i], XC[agg[i]]), (B[i] - sigma) / de[i], 0.8f);
    }
    __syncthreads();
  }
  const float* X0 = base(first);
  float* gx = tail[first].x;
  for (uint32_t i = t; i < desc[first].n; i += nt) gx[i] = X0[i];
}

}  // namespace

void launch_amg_tail(const AmgTailLevel* tail, int first, int nlev, size_t lds_bytes, hipStream_t s) {
  if (lds_bytes == 0) {
    hipLaunchKernelGGL(k_amg_tail, dim3(1), dim3(1024), 0, s, tail, first, nlev);
    return;
  }
  hipLaunchKernelGGL(k_amg_tail_lds, dim3(1), dim3(1024), lds_bytes, s, tail, first, nlev);
}
void launch_amg_tail_blob(const AmgTailLevel* tail, const TailBlobLevel* desc, const uint32_t* blob,
                          uint32_t blob_words, uint32_t vec_floats, int first, int nlev, const float* b_first,
                          uint32_t n_first, hipStream_t s) {
  const size_t lds = 4 * ((size_t)vec_floats + blob_words);
  if (lds > kTailLdsMax || blob_words % 4 || blob_words == 0) throw std::invalid_argument("AMG tail blob larger than the kernel's LDS image");
  if (n_first == 0 || 16 * (size_t)n_first > kTailLdsMax) throw std::invalid_argument("AMG tail: first level size");
  hipLaunchKernelGGL(k_amg_tail_blob, dim3(1), dim3(1024), lds, s, tail, desc, blob, blob_words, vec_floats, first,
                     nlev, b_first, n_first);
}
// Per-device kernel attributes: the LDS-resident tail kernels take more than
// the default 64 KiB of dynamic LDS.  The attribute belongs to the device that
// is current when it is set, so each device gets it once (std::call_once per
// device id; the in-process group runs one host thread per rank and device).
// Returns the dynamic-LDS budget of those kernels on this device: the smaller
// of kTailLdsMax and the device's opt-in per-block limit.
size_t init_kernel_attributes(int device) {
  constexpr int kMaxDevices = 64;
  static std::once_flag once[kMaxDevices];
  static hipError_t status[kMaxDevices];
  static size_t budget[kMaxDevices];
  if (device < 0 || device >= kMaxDevices) throw std::invalid_argument("HIP device id out of range");
  std::call_once(once[device], [device] {
    int optin = 0;
    hipError_t e = hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device);
    size_t lim = kTailLdsMax;
    if (e == hipSuccess && optin > 0) lim = std::min(lim, (size_t)optin);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_amg_tail_lds),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lim);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_amg_tail_blob),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lim);
    status[device] = e;
    budget[device] = lim;
  });
  if (status[device] != hipSuccess)
    throw std::runtime_error(std::string("setting the tail kernels' dynamic-LDS limit: ") +
                             hipGetErrorString(status[device]));
  return budget[device];
}

}  // namespace cfd2
