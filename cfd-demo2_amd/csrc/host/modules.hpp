// The opt-in post-processing modules: plain structs the Solver holds one of
// each.  Every method takes the solver as a const FlowView (flow_view.hpp) and
// whatever else it reads as an explicit argument; every device buffer lives in
// the module's own arenas, allocated by its first enabling call and cleared by
// its one reset method alone.  step() launches none of this.  One GPU only:
// the view does not exist on a distributed handle (Solver::view throws the
// module's kOneGpu).
#pragma once
#include <cstdint>
#include <vector>

#include "flow_view.hpp"
#include "topology.hpp"

namespace cfd2 {

// ---- frames on the device (render.cpp; kernels.hpp "render.hip") ----
// arena holds what depends on the polygons, view_arena the map and the image
// of the current view size; set_polygons(v, 0, ...) releases both.
struct Renderer {
  static constexpr const char* kOneGpu = "rendering runs on one GPU only: a distributed handle holds a part of the fields";
  DeviceArena arena, view_arena;
  RenderPolys polys{};          // N = 0: no polygons
  float bounds[4] = {};         // x0, y0, x1, y1 of the polygons' vertices (f32)
  uint32_t* list = nullptr;     // [N] the cells that take the wavefront path
  uint32_t* counts = nullptr;   // [4] listed cells, owned pixels, the auto range's two keys
  uint32_t* blockmm = nullptr;  // [2 * render_range_blocks(N)]
  RenderView view{};            // W = 0: no view
  size_t pixels = 0;            // pixels map / image hold
  uint32_t* map = nullptr;      // [H * W] owner or kRenderNone
  uint32_t* image = nullptr;    // [H * W] packed RGBA8
  uint32_t listed = 0;          // cells of the current view's list
  bool rendered = false;        // image holds a frame of the current view
  void release(const FlowView& flow);
  void set_polygons(const FlowView& flow, uint32_t nv, const double* vx, const double* vy, const uint32_t* off,
                    const uint32_t* idx);
  uint32_t set_view(const FlowView& flow, int32_t w, int32_t h, const double* box);  // returns the owned pixels
  // One frame in two halves, so that the solver can run the derived pass of
  // fields 4 and 5 between them (Solver::render): the argument checks, then the
  // launches.  derived: the vorticity / divergence cells of those two fields.
  void frame_check(const FlowView& flow, int32_t field, int32_t scalar_index) const;
  void frame(const FlowView& flow, int32_t field, int32_t scalar_index, const float* derived, const float* range,
             uint8_t* rgba, float* used);
  void owner(const FlowView& flow, uint32_t* out);
  // the last frame of the current view, for an overlay (what: the caller's name in the two messages)
  struct Frame {
    RenderView view;
    size_t pixels;
    const uint32_t* image;
  };
  Frame current_frame(const char* what) const;  // throws: no view, no frame of it yet
};

// ---- tracer particles (particles.cpp; kernels.hpp "particles.hip") ----
// mesh_arena holds the mesh upload, arena the particle set, frame_arena the
// stamped copy of a frame, seed_arena the seeds' staging buffer (grown when a
// seed call brings more than it holds, so a rake re-seeded every step
// allocates once); a new or released mesh frees the set too (its cells refer
// to the mesh it was located in).
struct Tracers {
  static constexpr const char* kOneGpu = "particles run on one GPU only: a distributed handle holds a part of the fields";
  DeviceArena mesh_arena, arena, frame_arena, seed_arena;
  ParticleMesh mesh{};                 // N = 0: no mesh
  ParticleSet set{};                   // n = 0: not enabled
  uint32_t hop_cap = 64;
  unsigned long long* stats_buf = nullptr; // [kParticleStats]
  uint32_t* frame = nullptr;           // [frame_pixels] packed RGBA8
  size_t frame_pixels = 0;
  float* seed_buf = nullptr;           // [2 * seed_cap]: x, then y
  uint32_t seed_cap = 0;
  std::vector<float> seed_host;        // the f32 seeds on their way up
  void free_set(const FlowView& flow);
  void need(const char* what, uint32_t first, uint32_t count) const;  // throws: not enabled, range
  // topo: wf, nface and fs_face (the face of every slot)
  void set_mesh(const FlowView& flow, const Topology& topo, uint32_t nv, const double* vx, const double* vy,
                const uint32_t* off, const uint32_t* idx, const uint32_t* fv1, const uint32_t* fv2);
  void enable(const FlowView& flow, uint32_t capacity, const cfd_particle_config* cfg);
  void seed(const FlowView& flow, uint32_t first, uint32_t count, const double* x, const double* y);
  void advance(const FlowView& flow, float dt);
  void get(const FlowView& flow, uint32_t first, uint32_t count, float* x, float* y, uint32_t* cell, uint32_t* status,
           float* age);
  void stats(const FlowView& flow, cfd_particle_stats* out);
  void render_particles(const FlowView& flow, const Renderer& r, uint32_t colour, uint8_t* rgba);
};

// ---- time statistics (timestats.cpp; kernels.hpp "timestats.hip") ----
struct TimeStats {
  static constexpr const char* kOneGpu = "time statistics run on one GPU only: a distributed handle holds a part of the fields";
  DeviceArena arena;
  double* planes = nullptr;     // [np * ld]; null: not enabled
  uint32_t np = 0;              // planes (tstats_planes)
  size_t ld = 0;                // plane stride: N rounded up to 32 doubles
  bool m2 = false;              // second moments
  bool scalars = false;         // the configuration asked for the scalar fields
  uint32_t nf = 0;              // fields the planes hold: the view's at enable (0 without scalars)
  double W = 0.0;               // total weight
  uint64_t samples = 0;
  void need(const char* what) const;  // throws: not enabled
  void enable(const FlowView& flow, const cfd_tstats_config* cfg);
  void disable(const FlowView& flow);
  void reset(const FlowView& flow);
  void accumulate(const FlowView& flow, float weight);
  int plane_of(int kind, int scalar_index, bool* covariance) const;  // throws: plane off, bad kind / index
  void get(const FlowView& flow, int kind, int scalar_index, double* out);
  void raw(const FlowView& flow, uint32_t plane, double* out, const double* in);  // one of the two is null
  void set_totals(const FlowView& flow, uint64_t samples_in, double W_in);
  void info(const FlowView& flow, uint64_t* samples_out, double* total_weight, uint32_t* planes_out) const;  // each may be null
};

// the decoding of the flow diagnostics' device result (diagnostics.cpp; sums:
// the six f64 patterns, m: the three maximum keys)
void flow_diag_decode(const uint64_t* sums, const uint64_t* m, uint32_t faces, cfd_flow_diag* out);

// ---- the monitor history (timestats.cpp): a ring of cap slots, sample k in slot k % cap ----
struct Monitor {
  static constexpr const char* kOneGpu = "the monitor runs on one GPU only: a distributed handle holds a part of the fields";
  DeviceArena arena;
  uint32_t cap = 0;             // 0: not enabled
  uint32_t P = 0, ns = 0;
  bool diag = false;
  uint64_t total = 0;           // samples ever recorded
  uint32_t* cells = nullptr;    // [P]
  float* time = nullptr;        // [cap][2] time, dt
  float* probe = nullptr;       // [cap][P][3 + ns]
  uint64_t* dres = nullptr;     // [cap][kMonitorDiagWords] (with diagnostics)
  std::vector<uint32_t> faces;  // [cap] the force region's faces at each record (host: the region is host state)
  void need(const char* what) const;
  void enable(const FlowView& flow, uint32_t capacity, uint32_t num_probes, const uint32_t* probe_cells, bool with_diag);
  void disable(const FlowView& flow);
  // record in two halves (Solver::monitor_record runs the flow diagnostics
  // between them when diag is set): the checks, then the launch.  diag_res: the
  // diagnostics' device result over `region`.
  void record_check(const FlowView& flow) const;
  void record(const FlowView& flow, const uint64_t* diag_res, const ForceRegion& region);
  void get(const FlowView& flow, uint64_t first, uint64_t count, float* time_out, float* dt, float* probes,
           cfd_flow_diag* diag_out);
  void count(const FlowView& flow, uint64_t* total_out, uint64_t* held) const;  // each may be null
  void info(const FlowView& flow, uint32_t* capacity, uint32_t* num_probes, uint32_t* scalar_fields,
            int32_t* with_diag) const;
};

// ---- wall surface distributions (surface.cpp; kernels.hpp "surface.hip") ----
// arena holds the face table, ch_arena the channel buffers (sample, mean, M2):
// the channel count follows the scalar fields, so those buffers are re-derived
// (and the statistics reset) by the first call after the view's surface_gen
// moved.  The total weight stays on the host.
struct SurfaceDist {
  static constexpr const char* kOneGpu =
      "surface distributions run on one GPU only: a distributed handle holds a part of the fields";
  DeviceArena arena, ch_arena;
  bool on = false;              // a surface exists (it may have no face)
  std::vector<uint32_t> face;   // indices into the wall-face list, ascending (cell, then slot)
  uint32_t* cell = nullptr;     // [n]
  uint32_t* slot = nullptr;     // [n]
  size_t ld = 0;                // channel stride: n rounded up to 64 (at least 64)
  uint32_t nch = 0;             // channels the buffers hold
  double* out = nullptr;        // [nch * ld]
  double* mean = nullptr;       // with statistics: [nch * ld] each
  double* m2 = nullptr;
  bool stats = false;
  double W = 0.0;               // total weight
  uint64_t samples = 0;
  uint64_t gen = 0;             // the view's surface_gen the channel buffers were derived for
  void need(const FlowView& flow, const char* what);  // throws: no surface; re-derives the channels
  void derive(const FlowView& flow);                  // the channel buffers for the current scalar count; statistics reset
  void clear(const FlowView& flow);
  SurfaceArgs args(const FlowView& flow) const;
  uint32_t select(const FlowView& flow, const std::vector<WallFace>& wall, double x0, double y0, double x1, double y1);
  void geometry(const FlowView& flow, const std::vector<WallFace>& wall, const Topology& topo, uint32_t* cell_out,
                uint32_t* slot_out, double* cx, double* cy, double* nx, double* ny, double* area, double* dist_e);
  void info(const FlowView& flow, cfd_surface_info* info_out);
  void sample(const FlowView& flow, double* sample_out);
  void stats_enable(const FlowView& flow, bool enable);
  void stats_reset(const FlowView& flow);
  void stats_accumulate(const FlowView& flow, double weight);
  void stats_get(const FlowView& flow, int kind, double* stats_out);
};

}  // namespace cfd2
