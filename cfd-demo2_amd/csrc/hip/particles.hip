// Tracer particles on the device (include/cfd2_amd.h "The tracers" is the
// contract; kernels.hpp "particles.hip").  One thread per particle in every
// kernel, 256-thread blocks, no LDS but the statistics' block fold.  All f32
// and compiled with contraction off, so positions, cells and ages are the bits
// of the numpy restatement (tests/particles_ref.py).
//
//   k_particles_locate   a seed's bin, the bin's cells from the largest index
//                        down, the renderer's closed fan test; the first owner
//                        found is the largest
//   k_particles_advance  the hop loop.  Per hop the lane gathers its cell's face
//                        slots (other, meta, the two vertex indices, 4
//                        coordinates; normals only on a wall hit).  Slot-major
//                        arrays are coalesced for neighbouring cells only, and
//                        particles are in no order, so these are per-lane
//                        gathers served by L2 (the mesh is read-only and small
//                        next to the state).  Lanes leave the loop one by one;
//                        the slot loop's loads are independent of each other,
//                        so a hop is one round trip, and the selection of the
//                        exit is predicated, not branched.
//   k_particles_stats    integer sums / maximum: wavefront trees, the block's
//                        four values, one atomic per value and block
//   k_particles_stamp    one 32-bit store per ALIVE particle in the view
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

// E of the edge (xa, ya) -> (xb, yb) at q ("edges" of the picture)
__device__ __forceinline__ float edge_at(float xa, float ya, float xb, float yb, float qx, float qy) {
  return (xb - xa) * (qy - ya) - (yb - ya) * (qx - xa);
}
// ... of the polygon edge from vertex `from` to vertex `to`: evaluated from the smaller index
__device__ __forceinline__ float poly_edge(const ParticleMesh& M, uint32_t from, uint32_t to, float qx, float qy) {
  const bool flip = to < from;
  const uint32_t a = flip ? to : from, b = flip ? from : to;
  const float e = edge_at(M.vx[a], M.vy[a], M.vx[b], M.vy[b], qx, qy);
  return flip ? -e : e;
}

// the closed fan test of cell c ("triangles" of the picture)
__device__ __forceinline__ bool cell_owns(const ParticleMesh& M, uint32_t c, float qx, float qy) {
  const uint32_t a = M.off[c], e = M.off[c + 1];
  if (e - a < 3u || e < a) return false;
  const uint32_t v0 = M.idx[a];
  for (uint32_t k = a + 1; k + 1 < e; ++k) {
    const uint32_t v1 = M.idx[k], v2 = M.idx[k + 1];
    if (poly_edge(M, v0, v1, M.vx[v2], M.vy[v2]) == 0.0f) continue;  // no area
    const float s1 = poly_edge(M, v0, v1, qx, qy), s2 = poly_edge(M, v1, v2, qx, qy), s3 = poly_edge(M, v2, v0, qx, qy);
    if ((s1 >= 0.0f && s2 >= 0.0f && s3 >= 0.0f) || (s1 <= 0.0f && s2 <= 0.0f && s3 <= 0.0f)) return true;
  }
  return false;
}

__global__ void __launch_bounds__(kBlock) k_particles_locate(ParticleMesh M, ParticleSet P, uint32_t first, uint32_t count,
                                                             const float* __restrict__ sx, const float* __restrict__ sy) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const uint32_t s = first + t;  // first + count <= P.n (the host checks)
  const float qx = sx[t], qy = sy[t];
  const uint32_t b = particle_bin(qy, M.by0, M.sy, M.nb) * M.nb + particle_bin(qx, M.bx0, M.sx, M.nb);
  const uint32_t lo = M.bin_off[b];
  uint32_t owner = kParticleNoCell;
  for (uint32_t q = M.bin_off[b + 1]; q > lo; --q) {  // ascending lists, walked from the top
    const uint32_t c = M.bin_cells[q - 1];
    if (cell_owns(M, c, qx, qy)) {
      owner = c;
      break;
    }
  }
  P.x[s] = qx;
  P.y[s] = qy;
  P.cell[s] = owner;
  P.status[s] = owner == kParticleNoCell ? CFD_PARTICLE_OUTSIDE : CFD_PARTICLE_ALIVE;
  P.age[s] = 0.0f;
  P.contacts[s] = 0u;
  P.hops[s] = 0u;
}

__global__ void __launch_bounds__(kBlock) k_particles_advance(ParticleMesh M, FaceSlots fs, const float2* __restrict__ u,
                                                              ParticleSet P, float dt, uint32_t hop_cap) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= P.n) return;
  uint32_t status = P.status[s];
  if (status != CFD_PARTICLE_ALIVE) {
    P.hops[s] = 0u;
    return;
  }
  const uint32_t N = M.N;
  float px = P.x[s], py = P.y[s], age = P.age[s], r = dt;
  uint32_t c = P.cell[s], contacts = P.contacts[s], hops = 0u, capped = 0u;
  float2 v = u[c];
  uint32_t skip = ~0u;  // the wall slot this traversal slides along
  for (;;) {
    const float ex = px + v.x * r, ey = py + v.y * r;
    const uint32_t nf = fs.nface[c];
    float bt = 2.0f, ht = 2.0f;  // any t is <= 1
    uint32_t bk = ~0u, hk = ~0u;  // the exit by segments, and by half-planes alone (the fallback)
    for (uint32_t k = 0; k < nf; ++k) {
      const size_t e = (size_t)k * N + c;
      const uint32_t sa = M.sa[e], b = M.sb[e], a = sa & ~kParticleSignBit;
      const float xa = M.vx[a], ya = M.vy[a], xb = M.vx[b], yb = M.vy[b];
      const bool neg = (sa & kParticleSignBit) != 0u;
      const float Ee = edge_at(xa, ya, xb, yb, ex, ey), Ep = edge_at(xa, ya, xb, yb, px, py);
      const float ge = neg ? -Ee : Ee, gp = neg ? -Ep : Ep;
      const float ha = v.x * (ya - py) - v.y * (xa - px), hb = v.x * (yb - py) - v.y * (xb - px);
      const bool across = (ha >= 0.0f && hb <= 0.0f) || (ha <= 0.0f && hb >= 0.0f);
      const float t = gp <= 0.0f ? 0.0f : gp / (gp - ge);
      const bool beyond = k != skip && ge < 0.0f;
      const bool take = beyond && across && t < bt;  // ties: the lowest slot
      bt = take ? t : bt;
      bk = take ? k : bk;
      const bool half = beyond && t < ht;
      ht = half ? t : ht;
      hk = half ? k : hk;
    }
    // a path along a face's line (a wall slide ends at the face's vertex) can miss every segment by a rounding
    if (bk == ~0u && hk != ~0u && !cell_owns(M, c, ex, ey)) {
      bt = ht;
      bk = hk;
    }
    if (bk == ~0u) {
      px = ex;
      py = ey;
      age = age + r;
      break;
    }
    if (hops == hop_cap) {
      capped = kParticleCapped;
      break;
    }
    const float step = r * bt;
    px = px + v.x * step;
    py = py + v.y * step;
    age = age + step;
    r = r - step;
    ++hops;
    const size_t e = (size_t)bk * N + c;
    const uint32_t btype = fs.meta[e] & kMetaBtypeMask;
    if (btype == 0u) {
      c = (uint32_t)fs.other[e];
      v = u[c];
      skip = ~0u;
    } else if (btype == 3u) {
      ++contacts;
      const float nx = fs.nx[e], ny = fs.ny[e];
      const float dn = v.x * nx + v.y * ny;
      v.x = v.x - dn * nx;
      v.y = v.y - dn * ny;
      skip = bk;
    } else {
      status = btype == 2u ? CFD_PARTICLE_EXITED_OUTLET : CFD_PARTICLE_EXITED_INLET;
      break;
    }
  }
  P.x[s] = px;
  P.y[s] = py;
  P.cell[s] = c;
  P.status[s] = status;
  P.age[s] = age;
  P.contacts[s] = contacts;
  P.hops[s] = hops | capped;
}

__global__ void __launch_bounds__(kBlock) k_particles_stats(ParticleSet P, unsigned long long* out) {
  using u64 = unsigned long long;
  __shared__ u64 l[kParticleStats][kBlock / 64];
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  u64 v[kParticleStats] = {};
  if (s < P.n) {
    const uint32_t st = P.status[s], h = P.hops[s];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) v[k] = st == k ? 1u : 0u;
    v[5] = P.contacts[s];
    v[6] = v[7] = h & ~kParticleCapped;
    v[8] = h >> 31;
  }
#pragma unroll
  for (int k = 0; k < kParticleStats; ++k) {
    const u64 w = k == 7 ? wave_max(v[k]) : wave_tree(v[k]);  // lane 0 holds either
    if (red_lane() == 0) l[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < kParticleStats) {
    const u64* q = l[threadIdx.x];
    if (threadIdx.x == 7) {
      const u64 m = block_of4_max(q);
      if (m) atomicMax(&out[7], m);
    } else {
      const u64 t = (q[0] + q[1]) + (q[2] + q[3]);
      if (t) atomicAdd(&out[threadIdx.x], t);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_particles_stamp(ParticleSet P, RenderView V, uint32_t colour,
                                                            uint32_t* __restrict__ rgba) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= P.n || P.status[s] != CFD_PARTICLE_ALIVE) return;
  const float fi = floorf((P.x[s] - V.x0) / V.dx), fj = floorf((V.y1 - P.y[s]) / V.dy);
  if (!(fi >= 0.0f && fi < (float)V.W && fj >= 0.0f && fj < (float)V.H)) return;  // also a NaN
  rgba[(size_t)(uint32_t)fj * V.W + (uint32_t)fi] = colour;
}

}  // namespace

void launch_particles_locate(const ParticleMesh& m, const ParticleSet& p, uint32_t first, uint32_t count, const float* x,
                             const float* y, hipStream_t s) {
  if (count) hipLaunchKernelGGL(k_particles_locate, dim3(grid_for(count)), dim3(kBlock), 0, s, m, p, first, count, x, y);
}

void launch_particles_advance(const ParticleMesh& m, const FaceSlots& fs, const float2* u, const ParticleSet& p, float dt,
                              uint32_t hop_cap, hipStream_t s) {
  if (p.n) hipLaunchKernelGGL(k_particles_advance, dim3(grid_for(p.n)), dim3(kBlock), 0, s, m, fs, u, p, dt, hop_cap);
}

void launch_particles_stats(const ParticleSet& p, unsigned long long* out, hipStream_t s) {
  if (p.n) hipLaunchKernelGGL(k_particles_stats, dim3(grid_for(p.n)), dim3(kBlock), 0, s, p, out);
}

void launch_particles_stamp(const ParticleSet& p, const RenderView& v, uint32_t colour, uint32_t* rgba, hipStream_t s) {
  if (p.n) hipLaunchKernelGGL(k_particles_stamp, dim3(grid_for(p.n)), dim3(kBlock), 0, s, p, v, colour, rgba);
}

}  // namespace cfd2
