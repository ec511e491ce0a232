// Tracer particles (include/cfd2_amd.h "The tracers"; kernels.hpp
// "particles.hip"): the mesh upload with its per-slot vertex pairs and the bin
// grid, the particle set, and the calls that seed, advance, count, read and
// stamp it.  Read-only on the solver's state by its type: the solver arrives as
// a const FlowView, pointers to const, and this file does not see the Solver.
// Every buffer lives in the module's own arenas.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "modules.hpp"

namespace cfd2 {

void Tracers::free_set(const FlowView& flow) {
  flow.sync();
  arena.release();
  frame_arena.release();
  seed_arena.release();
  set = ParticleSet{};
  stats_buf = nullptr;
  frame = nullptr;
  frame_pixels = 0;
  seed_buf = nullptr;
  seed_cap = 0;
}

void Tracers::set_mesh(const FlowView& flow, const Topology& topo, uint32_t nv, const double* vx, const double* vy,
                       const uint32_t* off, const uint32_t* idx, const uint32_t* fv1, const uint32_t* fv2) {
  CFD_HIP(hipSetDevice(flow.device));
  if (nv == 0) {
    free_set(flow);
    mesh_arena.release();
    mesh = ParticleMesh{};
    return;
  }
  if (!vx || !vy || !off || !idx || !fv1 || !fv2) throw std::invalid_argument("particle mesh: null array");
  if (nv >= kParticleSignBit) throw std::invalid_argument("particle mesh: num_vertices must be below 2^31");
  if (off[0] != 0) throw std::invalid_argument("particle mesh: cell_vertex_offsets[0] must be 0");
  for (uint32_t c = 0; c < flow.N; ++c)
    if (off[c + 1] < off[c])
      throw std::invalid_argument("particle mesh: cell_vertex_offsets decrease at cell " + std::to_string(c));
  const uint32_t total = off[flow.N];
  if (total >= (1u << 31)) throw std::invalid_argument("particle mesh: cell_vertex_offsets[N] must be below 2^31");
  for (uint32_t k = 0; k < total; ++k)
    if (idx[k] >= nv)
      throw std::invalid_argument("particle mesh: vertex index " + std::to_string(idx[k]) + " at entry " +
                                  std::to_string(k) + " outside [0, " + std::to_string(nv) + ")");
  std::vector<float> fx(nv), fy(nv);
  for (uint32_t v = 0; v < nv; ++v) fx[v] = (float)vx[v], fy[v] = (float)vy[v];
  // every face slot's vertex pair, found as consecutive vertices of the cell's
  // polygon; counter-clockwise polygons (the inner side is on the left)
  const int wf = topo.wf;
  std::vector<uint32_t> sa((size_t)wf * flow.N, 0u), sb((size_t)wf * flow.N, 0u);
  for (uint32_t c = 0; c < flow.N; ++c) {
    const uint32_t* p = idx + off[c];
    const uint32_t n = off[c + 1] - off[c];
    double area2 = 0.0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t a = p[j], b = p[j + 1 < n ? j + 1 : 0];
      area2 += vx[a] * vy[b] - vx[b] * vy[a];
    }
    if (!(area2 > 0.0))
      throw std::invalid_argument("particle mesh: the polygon of cell " + std::to_string(c) + " is not counter-clockwise");
    for (uint32_t k = 0; k < topo.nface[c]; ++k) {
      const size_t e = (size_t)k * flow.N + c;
      const uint32_t f = topo.fs_face[e];
      const uint32_t v1 = fv1[f], v2 = fv2[f];
      if (v1 >= nv || v2 >= nv || v1 == v2)
        throw std::invalid_argument("particle mesh: face " + std::to_string(f) + " needs two different vertices below " +
                                    std::to_string(nv));
      bool found = false, down = false;
      for (uint32_t j = 0; j < n && !found; ++j) {
        const uint32_t a = p[j], b = p[j + 1 < n ? j + 1 : 0];
        if ((a == v1 && b == v2) || (a == v2 && b == v1)) found = true, down = b < a;
      }
      if (!found)
        throw std::invalid_argument("particle mesh: the vertices of face " + std::to_string(f) +
                                    " are not consecutive in the polygon of cell " + std::to_string(c));
      sa[e] = std::min(v1, v2) | (down ? kParticleSignBit : 0u);
      sb[e] = std::max(v1, v2);
    }
  }
  // the bin grid over the f32 bounds of the polygons' vertices
  const float inf = std::numeric_limits<float>::infinity();
  float b[4] = {inf, inf, -inf, -inf};
  for (uint32_t k = 0; k < total; ++k) {
    const float x = fx[idx[k]], y = fy[idx[k]];
    b[0] = x < b[0] ? x : b[0];
    b[1] = y < b[1] ? y : b[1];
    b[2] = x > b[2] ? x : b[2];
    b[3] = y > b[3] ? y : b[3];
  }
  ParticleMesh m{};
  m.nb = std::min<uint32_t>(1024u, (uint32_t)std::ceil(std::sqrt((double)flow.N)));
  m.bx0 = b[0];
  m.by0 = b[1];
  m.sx = (b[2] - b[0]) / (float)m.nb;
  m.sy = (b[3] - b[1]) / (float)m.nb;
  if (!(m.sx > 0.0f) || !(m.sy > 0.0f) || !std::isfinite(m.sx) || !std::isfinite(m.sy))
    throw std::invalid_argument("particle mesh: the vertices' bounds are empty or not finite");
  const size_t nbins = (size_t)m.nb * m.nb;
  std::vector<uint32_t> boff(nbins + 1, 0u), range(4 * (size_t)flow.N);
  for (uint32_t c = 0; c < flow.N; ++c) {
    float cb[4] = {inf, inf, -inf, -inf};
    for (uint32_t k = off[c]; k < off[c + 1]; ++k) {
      const float x = fx[idx[k]], y = fy[idx[k]];
      cb[0] = x < cb[0] ? x : cb[0];
      cb[1] = y < cb[1] ? y : cb[1];
      cb[2] = x > cb[2] ? x : cb[2];
      cb[3] = y > cb[3] ? y : cb[3];
    }
    uint32_t* r = &range[4 * (size_t)c];
    r[0] = particle_bin(cb[0], m.bx0, m.sx, m.nb);
    r[1] = particle_bin(cb[1], m.by0, m.sy, m.nb);
    r[2] = particle_bin(cb[2], m.bx0, m.sx, m.nb);
    r[3] = particle_bin(cb[3], m.by0, m.sy, m.nb);
    for (uint32_t j = r[1]; j <= r[3]; ++j)
      for (uint32_t i = r[0]; i <= r[2]; ++i) ++boff[(size_t)j * m.nb + i + 1];
  }
  for (size_t q = 0; q < nbins; ++q) {
    if ((uint64_t)boff[q] + boff[q + 1] >= (1ull << 32)) throw std::invalid_argument("particle mesh: the bin lists overflow");
    boff[q + 1] += boff[q];
  }
  std::vector<uint32_t> bcells(boff[nbins]), cur(boff.begin(), boff.end() - 1);
  for (uint32_t c = 0; c < flow.N; ++c) {  // ascending cells: ascending lists
    const uint32_t* r = &range[4 * (size_t)c];
    for (uint32_t j = r[1]; j <= r[3]; ++j)
      for (uint32_t i = r[0]; i <= r[2]; ++i) bcells[cur[(size_t)j * m.nb + i]++] = c;
  }
  // validated: replace what was there (the particle set refers to the old mesh and goes with it)
  free_set(flow);
  mesh_arena.release();
  mesh = ParticleMesh{};
  m.vx = mesh_arena.upload(fx, flow.stream);
  m.vy = mesh_arena.upload(fy, flow.stream);
  m.off = mesh_arena.upload(std::vector<uint32_t>(off, off + flow.N + 1), flow.stream);
  m.idx = mesh_arena.upload(std::vector<uint32_t>(idx, idx + total), flow.stream);
  m.sa = mesh_arena.upload(sa, flow.stream);
  m.sb = mesh_arena.upload(sb, flow.stream);
  m.bin_off = mesh_arena.upload(boff, flow.stream);
  m.bin_cells = mesh_arena.upload(bcells, flow.stream);
  flow.sync();  // the uploads read host vectors that end here
  m.wf = wf;
  m.N = flow.N;
  mesh = m;
}

void Tracers::enable(const FlowView& flow, uint32_t capacity, const cfd_particle_config* cfg) {
  CFD_HIP(hipSetDevice(flow.device));
  if (capacity == 0) {
    free_set(flow);
    return;
  }
  if (mesh.N == 0) throw std::invalid_argument("particles: no mesh (cfd_particles_set_mesh)");
  if (capacity > (1u << 24)) throw std::invalid_argument("particles: capacity must be 0..2^24");
  int32_t cap = cfg ? cfg->hop_cap : 0;
  if (cap == 0) cap = 64;
  if (cap < 1 || cap > 65536) throw std::invalid_argument("particles: hop_cap must be 1..65536 (0: the default 64)");
  free_set(flow);
  ParticleSet p{};
  p.x = arena.alloc<float>(capacity);
  p.y = arena.alloc<float>(capacity);
  p.cell = arena.alloc<uint32_t>(capacity);
  p.status = arena.alloc<uint32_t>(capacity);
  p.age = arena.alloc<float>(capacity);
  p.contacts = arena.alloc<uint32_t>(capacity);
  p.hops = arena.alloc<uint32_t>(capacity);
  stats_buf = arena.alloc<unsigned long long>(kParticleStats);
  const size_t bytes = (size_t)capacity * 4;
  for (void* q : {(void*)p.x, (void*)p.y, (void*)p.age, (void*)p.status, (void*)p.contacts, (void*)p.hops})
    CFD_HIP(hipMemsetAsync(q, 0, bytes, flow.stream));  // EMPTY at (0, 0), age 0
  CFD_HIP(hipMemsetAsync(p.cell, 0xFF, bytes, flow.stream));
  flow.sync();
  p.n = capacity;
  set = p;
  hop_cap = (uint32_t)cap;
}

void Tracers::need(const char* what, uint32_t first, uint32_t count) const {
  if (set.n == 0) throw std::invalid_argument(std::string(what) + ": particles are not enabled (cfd_particles_enable)");
  if ((uint64_t)first + count > set.n)
    throw std::invalid_argument(std::string(what) + ": first + count exceeds the capacity " + std::to_string(set.n));
}

void Tracers::seed(const FlowView& flow, uint32_t first, uint32_t count, const double* x, const double* y) {
  need("particle seed", first, count);
  if (count == 0) return;
  if (!x || !y) throw std::invalid_argument("particle seed: null array");
  const Range range("particle seed");
  CFD_HIP(hipSetDevice(flow.device));
  if (count > seed_cap) {  // count <= the capacity <= 2^24
    flow.sync();
    seed_arena.release();
    seed_buf = nullptr;
    seed_cap = 0;
    seed_buf = seed_arena.alloc<float>(2 * (size_t)count);
    seed_cap = count;
  }
  seed_host.resize(2 * (size_t)count);
  for (uint32_t k = 0; k < count; ++k) seed_host[k] = (float)x[k], seed_host[(size_t)count + k] = (float)y[k];
  CFD_HIP(hipMemcpyAsync(seed_buf, seed_host.data(), 2 * (size_t)count * 4, hipMemcpyHostToDevice, flow.stream));
  launch_particles_locate(mesh, set, first, count, seed_buf, seed_buf + count, flow.stream);
  flow.check_launch("particle seed");
  flow.sync();  // the staging buffers are free for the next call
}

void Tracers::advance(const FlowView& flow, float dt) {
  need("particle advance", 0, 0);
  if (!(dt > 0.0f)) {
    if (!(flow.last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_particles_advance: dt <= 0 asks for the dt of the last cfd_step, and there was none");
    dt = flow.last_step_dt;
  }
  if (!std::isfinite(dt)) throw std::invalid_argument("cfd_particles_advance: dt must be finite");
  const Range range("particle advance");
  CFD_HIP(hipSetDevice(flow.device));
  launch_particles_advance(mesh, flow.fs, flow.u, set, dt, hop_cap, flow.stream);
  flow.check_launch("particle advance");
}

void Tracers::get(const FlowView& flow, uint32_t first, uint32_t count, float* x, float* y, uint32_t* cell,
                  uint32_t* status, float* age) {
  need("particle get", first, count);
  if (count == 0) return;
  CFD_HIP(hipSetDevice(flow.device));
  const size_t bytes = (size_t)count * 4;
  const std::pair<void*, const void*> io[] = {{x, set.x},           {y, set.y},    {cell, set.cell},
                                              {status, set.status}, {age, set.age}};
  for (const auto& q : io)
    if (q.first) CFD_HIP(hipMemcpyAsync(q.first, (const char*)q.second + (size_t)first * 4, bytes, hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

void Tracers::stats(const FlowView& flow, cfd_particle_stats* out) {
  need("particle stats", 0, 0);
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemsetAsync(stats_buf, 0, kParticleStats * sizeof(unsigned long long), flow.stream));
  launch_particles_stats(set, stats_buf, flow.stream);
  flow.check_launch("particle stats");
  unsigned long long h[kParticleStats] = {};
  CFD_HIP(hipMemcpyAsync(h, stats_buf, sizeof(h), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  *out = cfd_particle_stats{};
  for (int k = 0; k < 5; ++k) out->count[k] = h[k];
  out->wall_contacts = h[5];
  out->hops_total = h[6];
  out->hops_max = h[7];
  out->capped = h[8];
  out->capacity = set.n;
}

void Tracers::render_particles(const FlowView& flow, const Renderer& r, uint32_t colour, uint8_t* rgba) {
  need("render particles", 0, 0);
  const Renderer::Frame rf = r.current_frame("render particles");
  const Range range("render particles");
  CFD_HIP(hipSetDevice(flow.device));
  if (frame_pixels != rf.pixels) {
    flow.sync();
    frame_arena.release();
    frame = nullptr;
    frame_pixels = 0;
    frame = frame_arena.alloc<uint32_t>(rf.pixels);
    frame_pixels = rf.pixels;
  }
  const size_t bytes = rf.pixels * sizeof(uint32_t);
  CFD_HIP(hipMemcpyAsync(frame, rf.image, bytes, hipMemcpyDeviceToDevice, flow.stream));
  launch_particles_stamp(set, rf.view, colour, frame, flow.stream);
  flow.check_launch("render particles");
  CFD_HIP(hipMemcpyAsync(rgba, frame, bytes, hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

}  // namespace cfd2
