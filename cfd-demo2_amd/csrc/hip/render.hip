// Frames on the device (include/cfd2_amd.h "The picture" is the contract;
// kernels.hpp "render.hip"): the ownership map of a view -- which cell's fan
// covers each pixel centre, the largest index winning -- and, per frame, one
// thread per pixel that gathers the owner's value and stores one packed RGBA8
// word.  All f32 and compiled with contraction off, so the map and the image
// are the bits of the numpy restatement (tests/render_ref.py).
//
//   k_render_map_cells   thread per cell: the cell's pixel box; a box of at
//                        most kRenderInPlacePixels pixels is tested in place,
//                        a larger cell is appended to the list
//   k_render_map_listed  one wavefront (64 lanes) per listed cell, the lanes
//                        striding the box
//   k_render_map_finish  owner + 1 -> owner / kRenderNone in place, and the
//                        count of owned pixels
//   k_render_range       block minima / maxima of the value as keys, then
//                        k_block_fold (reduce_dev.hpp)
//   k_render_shade       the per-frame pass
// The map is built with atomicMax on owner + 1: an integer maximum is the same
// in any order, so the list's order (an atomicAdd cursor) changes nothing.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

struct PixBox {
  uint32_t i0, j0, bw, bh;  // first column and row, width and height (clipped to the image)
};

// The candidate pixels of cell c; false: none (fewer than 3 vertices, or a box
// off the image).  The clip is done in f32, before any conversion.
__device__ __forceinline__ bool render_box(const RenderPolys& P, const RenderView& V, uint32_t a, uint32_t e, PixBox& b) {
  if (e - a < 3u || e < a) return false;
  const float inf = __uint_as_float(0x7f800000u);
  float mnx = inf, mxx = -inf, mny = inf, mxy = -inf;
  for (uint32_t k = a; k < e; ++k) {
    const uint32_t v = P.idx[k];
    const float x = P.vx[v], y = P.vy[v];
    mnx = x < mnx ? x : mnx;
    mxx = x > mxx ? x : mxx;
    mny = y < mny ? y : mny;
    mxy = y > mxy ? y : mxy;
  }
  float fi0 = floorf((mnx - V.x0) / V.dx - 0.5f), fi1 = ceilf((mxx - V.x0) / V.dx - 0.5f);
  float fj0 = floorf((V.y1 - mxy) / V.dy - 0.5f), fj1 = ceilf((V.y1 - mny) / V.dy - 0.5f);
  const float wm = (float)(V.W - 1u), hm = (float)(V.H - 1u);
  fi0 = fi0 < 0.0f ? 0.0f : fi0;
  fj0 = fj0 < 0.0f ? 0.0f : fj0;
  fi1 = fi1 > wm ? wm : fi1;
  fj1 = fj1 > hm ? hm : fj1;
  if (!(fi0 <= fi1) || !(fj0 <= fj1)) return false;  // also a NaN bound
  b.i0 = (uint32_t)fi0;
  b.j0 = (uint32_t)fj0;
  b.bw = (uint32_t)fi1 - b.i0 + 1u;
  b.bh = (uint32_t)fj1 - b.j0 + 1u;
  return true;
}

// An edge in its canonical orientation (from the smaller vertex index).
struct Edge {
  float xa, ya, ex, ey;
  bool flip;
  __device__ __forceinline__ Edge(const RenderPolys& P, uint32_t from, uint32_t to) {
    flip = to < from;
    const uint32_t a = flip ? to : from, b = flip ? from : to;
    xa = P.vx[a];
    ya = P.vy[a];
    ex = P.vx[b] - xa;
    ey = P.vy[b] - ya;
  }
  __device__ __forceinline__ float at(float px, float py) const {
    const float e = ex * (py - ya) - ey * (px - xa);
    return flip ? -e : e;
  }
};

// Pixels first, first + stride, ... of the cell's box against every fan
// triangle; an owned pixel takes max(map, c + 1).
__device__ __forceinline__ void render_cell(const RenderPolys& P, const RenderView& V, uint32_t c, uint32_t a, uint32_t e,
                                            const PixBox& b, uint32_t* map, uint32_t first, uint32_t stride) {
  const uint32_t npx = b.bw * b.bh;
  const uint32_t v0 = P.idx[a];
  for (uint32_t k = a + 1; k + 1 < e; ++k) {
    const uint32_t v1 = P.idx[k], v2 = P.idx[k + 1];
    const Edge e1(P, v0, v1), e2(P, v1, v2), e3(P, v2, v0);
    if (e1.at(P.vx[v2], P.vy[v2]) == 0.0f) continue;  // no area
    for (uint32_t q = first; q < npx; q += stride) {
      const uint32_t i = b.i0 + q % b.bw, j = b.j0 + q / b.bw;
      const float px = V.x0 + ((float)i + 0.5f) * V.dx;
      const float py = V.y1 - ((float)j + 0.5f) * V.dy;
      const float s1 = e1.at(px, py), s2 = e2.at(px, py), s3 = e3.at(px, py);
      const bool own = (s1 >= 0.0f && s2 >= 0.0f && s3 >= 0.0f) || (s1 <= 0.0f && s2 <= 0.0f && s3 <= 0.0f);
      if (own) atomicMax(&map[(size_t)j * V.W + i], c + 1u);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_render_map_cells(RenderPolys P, RenderView V, uint32_t* map, uint32_t* list,
                                                             uint32_t* counts) {
  const uint32_t c = xcd_block() * kBlock + threadIdx.x;
  if (c >= P.N) return;
  const uint32_t a = P.off[c], e = P.off[c + 1];
  PixBox b;
  if (!render_box(P, V, a, e, b)) return;
  if (b.bw * b.bh > kRenderInPlacePixels) {
    list[atomicAdd(&counts[0], 1u)] = c;  // at most once per cell: the list holds N
    return;
  }
  render_cell(P, V, c, a, e, b, map, 0u, 1u);
}

__global__ void __launch_bounds__(kBlock) k_render_map_listed(RenderPolys P, RenderView V, uint32_t* map,
                                                              const uint32_t* list, uint32_t nlist) {
  const uint32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= nlist) return;
  const uint32_t c = list[w];
  const uint32_t a = P.off[c], e = P.off[c + 1];
  PixBox b;
  if (!render_box(P, V, a, e, b)) return;
  render_cell(P, V, c, a, e, b, map, lane, 64u);
}

__global__ void __launch_bounds__(kBlock) k_render_map_finish(uint32_t* map, uint32_t npix, uint32_t* covered) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  bool owned = false;
  if (q < npix) {
    const uint32_t m = map[q];
    owned = m != 0u;
    map[q] = m - 1u;  // 0 -> kRenderNone
  }
  const unsigned long long bal = __ballot(owned);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(covered, (uint32_t)__popcll(bal));
}

__device__ __forceinline__ float render_value(const RenderValue& f, uint32_t c) {
  if (f.mode == 3) return f.f[c];
  const float2 u = f.u[c];
  if (f.mode == 0) return sqrtf(u.x * u.x + u.y * u.y);
  return f.mode == 1 ? u.x : u.y;
}

// cfd_mesh_shader.wgsl:60-93 and the 8-bit rounding; R in the low byte
__device__ __forceinline__ uint32_t render_colour(float val, float lo, float hi) {
  const float r = hi - lo;
  const float safe = fabsf(r) < 1e-10f ? 1.0f : r;
  const float q = (val - lo) / safe;
  if (q != q) return 0xFF000000u;
  const float t = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
  float R, G, B;
  if (t < 0.5f) {
    const float s = t * 2.0f;
    R = 0.0f, G = s, B = 1.0f - s;
  } else {
    const float s = (t - 0.5f) * 2.0f;
    R = s, G = 1.0f - s, B = 0.0f;
  }
  const uint32_t rb = (uint32_t)(R * 255.0f + 0.5f), gb = (uint32_t)(G * 255.0f + 0.5f), bb = (uint32_t)(B * 255.0f + 0.5f);
  return rb | (gb << 8) | (bb << 16) | 0xFF000000u;
}

// 1024 cells per block, thread t its cells t, t + 256, ...
__global__ void __launch_bounds__(kBlock) k_render_range(RenderValue f, uint32_t N, uint32_t* blockmm) {
  __shared__ uint32_t lmm[2][kBlock / 64];
  uint32_t kmin = ~0u, kmax = 0u;
  for (uint32_t r = 0; r < 4; ++r) {
    const uint64_t ci = (uint64_t)blockIdx.x * 1024u + r * kBlock + threadIdx.x;
    if (ci < N) {
      const float v = render_value(f, (uint32_t)ci);
      if (v == v) {
        const uint32_t key = scalar_value_key(__float_as_uint(v));
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
    }
  }
  kmin = wave_min(kmin);
  kmax = wave_max(kmax);
  if ((threadIdx.x & 63) == 0) {
    lmm[0][threadIdx.x >> 6] = kmin;
    lmm[1][threadIdx.x >> 6] = kmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blockmm[2 * (size_t)blockIdx.x] = block_of4_min(lmm[0]);
    blockmm[2 * (size_t)blockIdx.x + 1] = block_of4_max(lmm[1]);
  }
}

// The frame: per pixel 4 B of the map read, 4 B stored, and the owner's value
// gathered.  Consecutive pixels of a row have the same or neighbouring owners,
// and the XCD remap (xcd_block) gives each XCD a contiguous band of rows, so
// the gathers of a band stay in that XCD's L2.
__global__ void __launch_bounds__(kBlock) k_render_shade(RenderValue f, const uint32_t* __restrict__ map, uint32_t npix,
                                                         const uint32_t* __restrict__ keys, float lo, float hi,
                                                         uint32_t* __restrict__ rgba) {
  const uint32_t q = xcd_block() * kBlock + threadIdx.x;
  if (q >= npix) return;
  if (keys) {
    const uint32_t kmin = keys[0], kmax = keys[1];
    if (kmin > kmax) {
      lo = 0.0f, hi = 1.0f;
    } else {
      lo = __uint_as_float(scalar_key_value(kmin));
      hi = __uint_as_float(scalar_key_value(kmax));
    }
  }
  const uint32_t c = map[q];
  rgba[q] = c == kRenderNone ? 0u : render_colour(render_value(f, c), lo, hi);
}

}  // namespace

void launch_render_map_cells(const RenderPolys& p, const RenderView& v, uint32_t* map, uint32_t* list, uint32_t* counts,
                             hipStream_t s) {
  if (p.N) hipLaunchKernelGGL(k_render_map_cells, dim3(grid_for(p.N)), dim3(kBlock), 0, s, p, v, map, list, counts);
}

void launch_render_map_listed(const RenderPolys& p, const RenderView& v, uint32_t* map, const uint32_t* list,
                              uint32_t nlist, hipStream_t s) {
  if (nlist)
    hipLaunchKernelGGL(k_render_map_listed, dim3((nlist + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, p, v, map,
                       list, nlist);
}

void launch_render_map_finish(uint32_t* map, uint32_t npix, uint32_t* covered, hipStream_t s) {
  if (npix) hipLaunchKernelGGL(k_render_map_finish, dim3(grid_for(npix)), dim3(kBlock), 0, s, map, npix, covered);
}

void launch_render_range(const RenderValue& f, uint32_t N, uint32_t* blockmm, uint32_t* keys, hipStream_t s) {
  const uint32_t nb = render_range_blocks(N);
  if (nb) hipLaunchKernelGGL(k_render_range, dim3(nb), dim3(kBlock), 0, s, f, N, blockmm);
  hipLaunchKernelGGL(k_block_fold<uint32_t>, dim3(1), dim3(kBlock), 0, s, blockmm, nb, 2u, 1u, keys);
}

void launch_render_shade(const RenderValue& f, const uint32_t* map, uint32_t npix, const uint32_t* keys, float lo,
                         float hi, uint32_t* rgba, hipStream_t s) {
  if (npix) hipLaunchKernelGGL(k_render_shade, dim3(grid_for(npix)), dim3(kBlock), 0, s, f, map, npix, keys, lo, hi, rgba);
}

}  // namespace cfd2
