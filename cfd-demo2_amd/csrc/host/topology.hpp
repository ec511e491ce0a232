// Mesh-derived host data: the static topology / geometry of the face slots and
// the wall-face list with its box selection rule.
#pragma once
#include <cstdint>
#include <vector>

#include "../../../include/cfd2_amd.h"
#include "dist.hpp"

namespace cfd2 {

// Mesh-derived static topology/geometry (init/mesh.rs + the per-slot geometric
// factors every face sweep needs), computed once on the host in f32 with the
// exact operation order of the WGSL expressions they replace.
struct Topology {
  uint32_t N = 0, F = 0;  // N = owned cells
  // distributed view (one GPU: c0 = 0, c1 = NG, no ghosts)
  uint32_t NG = 0, c0 = 0, c1 = 0;
  uint32_t npad = 0;           // N rounded up to 64: first upper-ghost local index
  uint32_t glo = 0, ghi = 0;   // ghosts below c0 / at or above c1
  std::vector<uint32_t> ghost; // ghost global ids, ascending
  RowWindow window() const { return RowWindow(c0, c1, ghost, glo); }
  // signed local index of a global cell id (owned or ghost)
  int32_t rel(uint32_t g) const { return window().rel(g); }
  int wf = 0;  // max faces per cell
  int ws = 0;  // max scalar row length (incl. diagonal)
  std::vector<float> vol;
  std::vector<uint32_t> nface;
  // face slots, [k*N + i]
  std::vector<int32_t> fs_other;
  std::vector<uint32_t> fs_meta;
  std::vector<uint32_t> fs_face;  // host only: face index of each slot
  std::vector<float> fs_area, fs_nx, fs_ny, fs_lam_s, fs_lam_f, fs_dist_a, fs_dist_e, fs_dvx,
      fs_dvy, fs_rx, fs_ry, fs_rox, fs_roy;
  // scalar CSR rows of the owned cells (init/mesh.rs:27-53), global columns,
  // and its ELL image [r*N + i] with signed local columns
  std::vector<uint32_t> srow, scol;
  uint32_t ld = 0;               // ELL slot stride (= npad)
  std::vector<int32_t> ell_col;  // [r*ld + i]
  std::vector<uint32_t> ell_len, ell_drank;  // [ld]
  bool use16 = false;            // every |col - row| < 2^15: ell_col16 valid
  std::vector<int16_t> ell_col16;
  std::vector<uint8_t> ell_len8, ell_drank8;
  // Coupled-matrix ELL (CoupledMatrix, kernels.hpp): the same rows with their
  // entries moved to aligned slots.  tmode[r] = the most frequent column - row
  // of slot r over the full rows; a row with fewer entries places each entry,
  // in CSR order, at the first slot still free whose mode is its delta, so
  // missing neighbours (walls) leave gaps instead of shifting the rest of the
  // row, and 4 consecutive rows keep 4 consecutive columns per slot.  Gaps and
  // trailing slots hold the virtual column row + tmode[r] (clamped into the
  // vectors' range; never accumulated).  Position layout when ws > 8 (the
  // Voronoi meshes).
  std::vector<int32_t> tmode;
  std::vector<uint8_t> tslot;    // [nnz] slot of CSR entry k
  std::vector<int32_t> tcol;     // [r*ld + i]
  std::vector<int16_t> tcol16;   // (use16)
  std::vector<uint16_t> tlg;     // [ld] slots in use | gap mask << 8
  std::vector<uint8_t> tdrank8;  // [ld] slot of the diagonal
};

// Throws std::invalid_argument on inconsistent meshes.
void build_topology(const cfd_mesh_view& m, Topology& t);
// Owned range [c0, c1) of a distributed rank, ghosts from the face neighbours.
void build_topology(const cfd_mesh_view& m, Topology& t, uint32_t c0, uint32_t c1);

// every wall face of the WHOLE mesh, f64 centre
struct WallFace {
  double cx, cy;
  uint32_t cell;      // global owner cell
  uint32_t slot;      // its slot in the owner's face list
};
// the selection rule of a box of wall faces (the force region and the surface
// share it): indices into wall, ascending, of the faces whose f64 centre lies
// in the closed box; none for an inverted box (x1 < x0)
std::vector<uint32_t> wall_faces_in_box(const std::vector<WallFace>& wall, double x0, double y0, double x1, double y1);

// The force region (Solver::set_force_region): the wall faces the force sums,
// the wall-motion sums and the monitor's records run over.
struct ForceRegion {
  bool on = false;               // some face selected: every rank runs the same kernel form
  uint32_t faces = 0;            // selected wall faces, whole mesh
  uint64_t gen = 0;              // set_force_region calls
  double box[4] = {0, 0, -1, 0};
  uint16_t* mask = nullptr;      // [N] selected wall slots, in the solver's arena (first non-empty region)
  bool holds(double cx, double cy) const { return cx >= box[0] && cx <= box[2] && cy >= box[1] && cy <= box[3]; }
};

// every inlet and wall face of the mesh, ascending face index (boundary_velocity.hpp)
struct BndFace {
  uint32_t face;
  uint32_t cell, slot;
  uint32_t btype;     // 1 inlet, 3 wall
  double nx, ny;      // the f64 face normal (its sign does not matter here)
  double cx, cy;      // the f64 face centre
};
std::vector<BndFace> boundary_faces(const cfd_mesh_view& m);  // after build_topology checked the mesh

}  // namespace cfd2
