// Frames on the device (include/cfd2_amd.h "The picture"; kernels.hpp
// "render.hip"): the polygons are uploaded once, the ownership map is built
// once per view, and a frame is the range reduction (auto range only), one
// shade launch and the copy of 4 W H bytes.  Read-only on the solver's state;
// every buffer lives in the renderer's own two arenas.
#include <cmath>
#include <cstring>
#include <limits>

#include "solver_impl.hpp"

namespace cfd2 {

namespace {
const char* kOneGpu = "rendering runs on one GPU only: a distributed handle holds a part of the fields";
}

void Solver::render_release() {
  sync();
  rd_arena.release();
  rd_view_arena.release();
  rd_polys = RenderPolys{};
  rd_view = RenderView{};
  rd_list = rd_counts = rd_blockmm = rd_map = rd_image = nullptr;
  rd_pixels = 0;
  rd_listed = 0;
  rd_rendered = false;
}

void Solver::render_set_polygons(uint32_t nv, const double* vx, const double* vy, const uint32_t* off,
                                 const uint32_t* idx) {
  if (dist()) throw std::invalid_argument(kOneGpu);
  CFD_HIP(hipSetDevice(device));
  if (nv == 0) {
    render_release();
    return;
  }
  if (!vx || !vy || !off || !idx) throw std::invalid_argument("render polygons: null array");
  if (off[0] != 0) throw std::invalid_argument("render polygons: cell_vertex_offsets[0] must be 0");
  for (uint32_t c = 0; c < N; ++c)
    if (off[c + 1] < off[c])
      throw std::invalid_argument("render polygons: cell_vertex_offsets decrease at cell " + std::to_string(c));
  const uint32_t total = off[N];
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
  render_release();
  rd_polys.vx = rd_arena.upload(fx, stream);
  rd_polys.vy = rd_arena.upload(fy, stream);
  rd_polys.off = rd_arena.upload(std::vector<uint32_t>(off, off + N + 1), stream);
  rd_polys.idx = rd_arena.upload(std::vector<uint32_t>(idx, idx + total), stream);
  rd_list = rd_arena.alloc<uint32_t>(N);
  rd_counts = rd_arena.alloc<uint32_t>(4);
  rd_blockmm = rd_arena.alloc<uint32_t>(2 * (size_t)render_range_blocks(N));
  sync();  // the uploads read host vectors that end here
  rd_polys.N = N;
  std::memcpy(rd_bounds, b, sizeof(b));
}

uint32_t Solver::render_set_view(int32_t w, int32_t h, const double* box) {
  if (dist()) throw std::invalid_argument(kOneGpu);
  if (rd_polys.N == 0) throw std::invalid_argument("render view: no polygons (cfd_render_set_polygons)");
  rd_view = RenderView{};  // a refused or failed call leaves no view
  rd_rendered = false;
  if (w < 1 || w > 8192 || h < 1 || h > 8192)
    throw std::invalid_argument("render view: width and height must be 1..8192");
  float b[4];
  for (int k = 0; k < 4; ++k) b[k] = box ? (float)box[k] : rd_bounds[k];
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
  CFD_HIP(hipSetDevice(device));
  const size_t npix = (size_t)w * (size_t)h;
  if (npix != rd_pixels) {
    sync();
    rd_view_arena.release();
    rd_map = rd_image = nullptr;
    rd_pixels = 0;
    rd_map = rd_view_arena.alloc<uint32_t>(npix);
    rd_image = rd_view_arena.alloc<uint32_t>(npix);
    rd_pixels = npix;
  }
  CFD_HIP(hipMemsetAsync(rd_map, 0, npix * sizeof(uint32_t), stream));
  CFD_HIP(hipMemsetAsync(rd_counts, 0, 2 * sizeof(uint32_t), stream));
  launch_render_map_cells(rd_polys, v, rd_map, rd_list, rd_counts, stream);
  check_launch("render map (cells)");
  uint32_t hc[2] = {0, 0};
  CFD_HIP(hipMemcpyAsync(hc, rd_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  sync();
  if (hc[0] > N) throw std::runtime_error("render map: the cell list overflowed");
  rd_listed = hc[0];
  launch_render_map_listed(rd_polys, v, rd_map, rd_list, rd_listed, stream);
  launch_render_map_finish(rd_map, (uint32_t)npix, rd_counts + 1, stream);
  check_launch("render map");
  CFD_HIP(hipMemcpyAsync(hc, rd_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  sync();
  rd_view = v;
  return hc[1];
}

void Solver::render(int32_t field, int32_t scalar_index, const float* range, uint8_t* rgba, float* used) {
  if (dist()) throw std::invalid_argument(kOneGpu);
  if (rd_polys.N == 0) throw std::invalid_argument("render: no polygons (cfd_render_set_polygons)");
  if (rd_view.W == 0) throw std::invalid_argument("render: no view (cfd_render_set_view)");
  if (field < 0 || field > 6)
    throw std::invalid_argument("render: field must be 0 (speed), 1 (u.x), 2 (u.y), 3 (p), 4 (vorticity), 5 (divergence) "
                                "or 6 (scalar)");
  if (field == 6) scalar_check(scalar_index);
  const Range rr("render");
  CFD_HIP(hipSetDevice(device));
  RenderValue f{};
  if (field <= 2) {
    f.mode = field;
    f.u = S().u;
  } else {
    f.mode = 3;
    if (field == 3) {
      f.f = S().p;
    } else if (field == 6) {
      f.f = sc_field[scalar_index].phi;
    } else {
      flow_diagnostics(nullptr, true);  // the derived pass, its field outputs on
      f.f = field == 4 ? diag_omega : diag_div;
    }
  }
  uint32_t* keys = nullptr;
  if (!range) {
    keys = rd_counts + 2;
    launch_render_range(f, N, rd_blockmm, keys, stream);
  }
  launch_render_shade(f, rd_map, (uint32_t)rd_pixels, keys, range ? range[0] : 0.0f, range ? range[1] : 0.0f, rd_image,
                      stream);
  check_launch("render");
  uint32_t hk[2] = {0, 0};
  if (keys) CFD_HIP(hipMemcpyAsync(hk, keys, sizeof(hk), hipMemcpyDeviceToHost, stream));
  CFD_HIP(hipMemcpyAsync(rgba, rd_image, rd_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  sync();
  rd_rendered = true;
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

void Solver::render_owner(uint32_t* out) {
  if (dist()) throw std::invalid_argument(kOneGpu);
  if (rd_polys.N == 0) throw std::invalid_argument("render owner: no polygons (cfd_render_set_polygons)");
  if (rd_view.W == 0) throw std::invalid_argument("render owner: no view (cfd_render_set_view)");
  CFD_HIP(hipSetDevice(device));
  CFD_HIP(hipMemcpyAsync(out, rd_map, rd_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  sync();
}

}  // namespace cfd2
