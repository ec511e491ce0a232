// Frames on the device (include/cfd2_amd.h "The picture"; kernels.hpp
// "render.hip"): the polygons are uploaded once, the ownership map is built
// once per view, and a frame is the range reduction (auto range only), one
// shade launch and the copy of 4 W H bytes.  Read-only on the solver's state by
// its type: the solver arrives as a const FlowView, pointers to const, and this
// file does not see the Solver.  Every buffer lives in the renderer's two arenas.
#include <cmath>
#include <cstring>
#include <limits>

#include "modules.hpp"

namespace cfd2 {

void Renderer::release(const FlowView& flow) {
  flow.sync();
  arena.release();
  view_arena.release();
  polys = RenderPolys{};
  view = RenderView{};
  list = counts = blockmm = map = image = nullptr;
  pixels = 0;
  listed = 0;
  rendered = false;
}

void Renderer::set_polygons(const FlowView& flow, uint32_t nv, const double* vx, const double* vy, const uint32_t* off,
                            const uint32_t* idx) {
  CFD_HIP(hipSetDevice(flow.device));
  if (nv == 0) {
    release(flow);
    return;
  }
  if (!vx || !vy || !off || !idx) throw std::invalid_argument("render polygons: null array");
  if (off[0] != 0) throw std::invalid_argument("render polygons: cell_vertex_offsets[0] must be 0");
  for (uint32_t c = 0; c < flow.N; ++c)
    if (off[c + 1] < off[c])
      throw std::invalid_argument("render polygons: cell_vertex_offsets decrease at cell " + std::to_string(c));
  const uint32_t total = off[flow.N];
  if (total >= (1u << 31)) throw std::invalid_argument("render polygons: cell_vertex_offsets[N] must be below 2^31");
  for (uint32_t k = 0; k < total; ++k)
    if (idx[k] >= nv)
      throw std::invalid_argument("render polygons: vertex index " + std::to_string(idx[k]) + " at entry " +
                                  std::to_string(k) + " outside [0, " + std::to_string(nv) + ")");
  std::vector<float> fx(nv), fy(nv);
  for (uint32_t v = 0; v < nv; ++v) fx[v] = (float)vx[v], fy[v] = (float)vy[v];
  // compute_bounds over the polygons' vertices (a NaN is ignored by the comparisons)
  const float inf = std::numeric_limits<float>::infinity();
  float b[4] = {inf, inf, -inf, -inf};
  for (uint32_t k = 0; k < total; ++k) {
    const float x = fx[idx[k]], y = fy[idx[k]];
    b[0] = x < b[0] ? x : b[0];
    b[1] = y < b[1] ? y : b[1];
    b[2] = x > b[2] ? x : b[2];
    b[3] = y > b[3] ? y : b[3];
  }
  release(flow);
  polys.vx = arena.upload(fx, flow.stream);
  polys.vy = arena.upload(fy, flow.stream);
  polys.off = arena.upload(std::vector<uint32_t>(off, off + flow.N + 1), flow.stream);
  polys.idx = arena.upload(std::vector<uint32_t>(idx, idx + total), flow.stream);
  list = arena.alloc<uint32_t>(flow.N);
  counts = arena.alloc<uint32_t>(4);
  blockmm = arena.alloc<uint32_t>(2 * (size_t)render_range_blocks(flow.N));
  flow.sync();  // the uploads read host vectors that end here
  polys.N = flow.N;
  std::memcpy(bounds, b, sizeof(b));
}

uint32_t Renderer::set_view(const FlowView& flow, int32_t w, int32_t h, const double* box) {
  if (polys.N == 0) throw std::invalid_argument("render view: no polygons (cfd_render_set_polygons)");
  view = RenderView{};  // a refused or failed call leaves no view
  rendered = false;
  if (w < 1 || w > 8192 || h < 1 || h > 8192)
    throw std::invalid_argument("render view: width and height must be 1..8192");
  float b[4];
  for (int k = 0; k < 4; ++k) b[k] = box ? (float)box[k] : bounds[k];
  for (float v : b)
    if (!std::isfinite(v)) throw std::invalid_argument("render view: the box must be finite");
  if (!(b[2] > b[0]) || !(b[3] > b[1])) throw std::invalid_argument("render view: the box needs x1 > x0 and y1 > y0");
  RenderView v{};
  v.W = (uint32_t)w;
  v.H = (uint32_t)h;
  v.x0 = b[0];
  v.y1 = b[3];
  v.dx = (b[2] - b[0]) / (float)w;
  v.dy = (b[3] - b[1]) / (float)h;
  if (!(v.dx > 0.0f) || !(v.dy > 0.0f) || !std::isfinite(v.dx) || !std::isfinite(v.dy))
    throw std::invalid_argument("render view: the box is too small or too large for this image size");
  const Range range("render map");
  CFD_HIP(hipSetDevice(flow.device));
  const size_t npix = (size_t)w * (size_t)h;
  if (npix != pixels) {
    flow.sync();
    view_arena.release();
    map = image = nullptr;
    pixels = 0;
    map = view_arena.alloc<uint32_t>(npix);
    image = view_arena.alloc<uint32_t>(npix);
    pixels = npix;
  }
  CFD_HIP(hipMemsetAsync(map, 0, npix * sizeof(uint32_t), flow.stream));
  CFD_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), flow.stream));
  launch_render_map_cells(polys, v, map, list, counts, flow.stream);
  flow.check_launch("render map (cells)");
  uint32_t hc[2] = {0, 0};
  CFD_HIP(hipMemcpyAsync(hc, counts, sizeof(uint32_t), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  if (hc[0] > flow.N) throw std::runtime_error("render map: the cell list overflowed");
  listed = hc[0];
  launch_render_map_listed(polys, v, map, list, listed, flow.stream);
  launch_render_map_finish(map, (uint32_t)npix, counts + 1, flow.stream);
  flow.check_launch("render map");
  CFD_HIP(hipMemcpyAsync(hc, counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  view = v;
  return hc[1];
}

void Renderer::frame_check(const FlowView& flow, int32_t field, int32_t scalar_index) const {
  if (polys.N == 0) throw std::invalid_argument("render: no polygons (cfd_render_set_polygons)");
  if (view.W == 0) throw std::invalid_argument("render: no view (cfd_render_set_view)");
  if (field < 0 || field > 6)
    throw std::invalid_argument("render: field must be 0 (speed), 1 (u.x), 2 (u.y), 3 (p), 4 (vorticity), 5 (divergence) "
                                "or 6 (scalar)");
  if (field == 6) flow.scalar_check(scalar_index);
}

void Renderer::frame(const FlowView& flow, int32_t field, int32_t scalar_index, const float* derived, const float* range,
                     uint8_t* rgba, float* used) {
  frame_check(flow, field, scalar_index);
  CFD_HIP(hipSetDevice(flow.device));
  RenderValue f{};
  if (field <= 2) {
    f.mode = field;
    f.u = flow.u;
  } else {
    f.mode = 3;
    if (field == 3) {
      f.f = flow.p;
    } else if (field == 6) {
      f.f = flow.field[scalar_index].phi;
    } else {
      f.f = derived;
    }
  }
  uint32_t* keys = nullptr;
  if (!range) {
    keys = counts + 2;
    launch_render_range(f, flow.N, blockmm, keys, flow.stream);
  }
  launch_render_shade(f, map, (uint32_t)pixels, keys, range ? range[0] : 0.0f, range ? range[1] : 0.0f, image,
                      flow.stream);
  flow.check_launch("render");
  uint32_t hk[2] = {0, 0};
  if (keys) CFD_HIP(hipMemcpyAsync(hk, keys, sizeof(hk), hipMemcpyDeviceToHost, flow.stream));
  CFD_HIP(hipMemcpyAsync(rgba, image, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  rendered = true;
  if (!used) return;
  if (range) {
    used[0] = range[0];
    used[1] = range[1];
  } else if (hk[0] > hk[1]) {
    used[0] = 0.0f;
    used[1] = 1.0f;
  } else {
    const uint32_t lo = scalar_key_value(hk[0]), hi = scalar_key_value(hk[1]);
    std::memcpy(&used[0], &lo, 4);
    std::memcpy(&used[1], &hi, 4);
  }
}

void Renderer::owner(const FlowView& flow, uint32_t* out) {
  if (polys.N == 0) throw std::invalid_argument("render owner: no polygons (cfd_render_set_polygons)");
  if (view.W == 0) throw std::invalid_argument("render owner: no view (cfd_render_set_view)");
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemcpyAsync(out, map, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

Renderer::Frame Renderer::current_frame(const char* what) const {
  if (view.W == 0) throw std::invalid_argument(std::string(what) + ": no view (cfd_render_set_view)");
  if (!rendered) throw std::invalid_argument(std::string(what) + ": no frame of this view yet (cfd_render)");
  return Frame{view, pixels, image};
}

}  // namespace cfd2
