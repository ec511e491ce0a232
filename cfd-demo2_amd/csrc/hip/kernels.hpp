// Kernel argument blocks + launch wrappers for the gfx950 HIP kernels.
//
// Data layout in HBM:
//  * per-cell arrays are SoA (float / float2) indexed by cell;
//  * per-(cell, face-slot) static geometry and per-(cell, neighbour-slot)
//    matrix blocks are ELL "slot-major": element (slot k, cell i) at k*N + i,
//    so lane-i accesses of one slot are fully coalesced across a wavefront;
//  * the coupled 3N x 3N matrix is stored as compressed 3x3 blocks: the
//    reference CSR (init/linear_solver/mod.rs:180-216) always holds
//    A_uu == A_vv, A_uv == A_vu == 0, A_up == A_pu, A_vp == A_pv per
//    off-diagonal block (coupled_assembly_merged.wgsl:221-333), so two float2
//    per block -- cval_a {c, pp} and cval_g {gx, gy} -- reproduce every CSR
//    entry bit-for-bit.  The Schur predict/correct kernels read cval_g only.
//  * Krylov basis vectors are stored unnormalised (W_i) with their scale
//    binv[i]; every consumer forms V_i[e] = binv[i] * W_i[e] (one f32 multiply,
//    the same rounding as the reference's `scale` pass, which is thereby gone).
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../../include/cfd2_amd.h"

namespace cfd2 {

// meta bits of a face slot
constexpr uint32_t kMetaBtypeMask = 0x3u;      // 0 internal, 1 inlet, 2 outlet, 3 wall
constexpr uint32_t kMetaOwner = 1u << 2;       // face_owner == this cell
constexpr uint32_t kMetaDegen = 1u << 3;       // d_c + d_o <= 1e-6 (lambda fallback 0.5)
constexpr uint32_t kMetaFluxFlip = 1u << 4;    // normal_flux = -stored normal
constexpr uint32_t kMetaRankShift = 8;         // scalar-row rank of the neighbour (0xFF boundary)
constexpr uint32_t kMetaTSlotShift = 16;       // its slot in the coupled-matrix ELL (Topology::tslot)

// Canonical reduction order (rank-invariant; mirrors oracle/oracle.cpp).  A
// sum over cells is ONE fixed binary tree over global cell indices:
//   chunk    256 consecutive cells [256k, 256k + 256): pairwise tree over the
//            256 cell terms (missing cells: +0).  The cell term of a dot of
//            3-component vectors (3 floats per cell) is (x_u y_u + x_v y_v) +
//            x_p y_p.  GPU: a wavefront's 64 consecutive cells by a shuffle tree
//            (strides 1, 2, ..., 32), then the chunk's 4 quarters pairwise
//   segment  G = 2^g consecutive chunks: pairwise tree over G chunk slots
//            (chunks past the end: +0).  g depends on the GLOBAL cell count
//            only: g = clamp(floor(log2(N / 16384)), 0, 8)
//   total    pairwise tree over the segment values, padded with +0 to a power
//            of two.
// A rank owns whole segments (partition_starts), so each segment value is
// computed by one rank and the total from the all-gathered segment values: R
// ranks produce exactly the bits of one GPU.  The chunk kernels combine the
// 4 chunks of their block as far as a segment allows: they write "units" of
// U = min(G, 4) chunks (the first log2(U) levels of the segment tree), so a
// segment is G / U units.
constexpr uint32_t kRedChunkCells = 256;
constexpr uint32_t kRedMaxSegLog2 = 8;
constexpr uint32_t kRedMaxSegments = 4096;  // the total's tree runs in LDS (N <= 268 M cells)
// A 256-thread block of a chunk kernel takes 4 chunks: thread t of block b
// handles cells b * kRedBlockCells + q * kRedChunkCells + t, q = 0..3.
constexpr uint32_t kRedBlockCells = 4 * kRedChunkCells;
// Its grid.  ceil(ceil(N / 256) / 4) == ceil(N / 1024) for every N, and the
// 32-bit N + 1023 cannot wrap: the solver refuses meshes above 2^28 cells
// (kRedMaxSegments segments of at most 2^16 cells).
inline uint32_t red_blocks(uint32_t N) { return (N + kRedBlockCells - 1) / kRedBlockCells; }

struct RedGeom {
  uint32_t g = 0;          // log2 chunks per segment
  uint32_t G = 1;          // chunks per segment
  uint32_t U = 1;          // chunks per unit written by the chunk kernels: min(G, 4)
  uint64_t seg_cells = 256;
  uint32_t nchunks = 0;    // global chunks
  uint32_t nseg = 0;       // global segments
};
inline RedGeom red_geom(uint64_t nglob) {
  RedGeom r;
  uint32_t g = 0;
  while (g < kRedMaxSegLog2 && (nglob >> (g + 1)) >= 16384u) ++g;
  r.g = g;
  r.G = 1u << g;
  r.U = r.G < 4 ? r.G : 4;
  r.seg_cells = (uint64_t)kRedChunkCells << g;
  r.nchunks = (uint32_t)((nglob + kRedChunkCells - 1) / kRedChunkCells);
  r.nseg = (uint32_t)((r.nchunks + r.G - 1) / r.G);
  return r;
}

// Where a chunk kernel leaves the unit partials of its f64 sums (reduce_dev.hpp
// sum_accumulate / sum_store): sum f's unit k at partial[f * np + k].
struct SumOut {
  uint32_t U;       // chunks per unit (RedGeom::U)
  uint32_t np;      // unit partials per sum (the stride between sums)
  double* partial;  // [sums * np]
};

// Source of a reduction's segment values for the kernels that finish it
// (the total's tree).  One GPU: unit partials p[v * stride + k], k < nchunks
// (here: units), G units per segment; the segment trees are built from them.  Distributed: the all-gathered
// segment values, rank q's block [q][v][local segment] of nvec x stride
// values; seg_src[s] = (q << 20) | local segment of global segment s.
template <class T>
struct RedSrcT {
  const T* p = nullptr;
  uint32_t stride = 0;
  uint32_t nchunks = 0;
  uint32_t G = 1;
  uint32_t nseg = 0;
  uint32_t nvec = 1;
  const uint32_t* seg_src = nullptr;
  // 0: the canonical tree.  Reference order (test mode, Solver::ref_red): 1
  // one thread adds the nchunks group partials in order (reduce_final,
  // gmres_ops.wgsl:257-262); 2 lanes t < 64 add partials t, t + 64, ...,
  // then the 64-wide halving tree (reduce_dots_cgs, gmres_cgs.wgsl:97-118)
  uint32_t order = 0;
};
using RedSrc = RedSrcT<float>;
using RedSrcD = RedSrcT<double>;

// Local cell numbering: every per-cell device pointer points at the first
// OWNED cell; neighbour indices are signed offsets from it.  On one GPU they
// are the global indices; on a distributed rank ghosts of lower ranks sit at
// [-glo, 0) and ghosts of higher ranks at [npad, npad + ghi) (npad = owned
// count rounded up to 64), so local order == global order.
constexpr int32_t kNoCell = INT32_MIN;  // boundary face: no neighbour

struct FaceSlots {  // ELL [k*N + i], k < wf
  const int32_t* other;  // neighbour (signed local index) or kNoCell
  const uint32_t* meta;
  const float* area;
  const float* nx;  // normal oriented out of this cell
  const float* ny;
  const float* lam_s;   // lambda from this cell's side (d_o / (d_c + d_o))
  const float* lam_f;   // lambda from the owner's side (flux interpolation)
  const float* dist_a;  // max(|d . n|, 1e-6)
  const float* dist_e;  // |other_center - center|
  const float* dvx;     // other_center - center
  const float* dvy;
  const float* rx;      // f_center - center
  const float* ry;
  const float* rox;     // f_center - other_center
  const float* roy;
  const uint32_t* nface;  // [N]
  int wf;
};

struct StateView {
  float2* u;
  float* p;
  float* dp;
  float2* gp;
};

struct PrepareArgs {
  uint32_t N;
  cfd_constants c;
  FaceSlots fs;
  const float* vol;
  StateView st;       // read (snapshot)
  float* dp_out;      // new d_p
  float2* gp_out;     // new grad_p
  float* flux_s;      // [k*N + i] oriented flux
  float2* grad_u;
  float2* grad_v;
};

struct AssembleArgs {
  uint32_t N;
  uint32_t ld;             // scalar-row ELL slot stride
  cfd_constants c;
  FaceSlots fs;
  const float* vol;
  StateView st;            // current iterate (d_p already refreshed)
  const float2* u_old;     // state_old.u
  const float2* u_old_old; // state_old_old.u
  const float* flux_s;
  const float2* grad_u;
  const float2* grad_v;
  const uint32_t* srank_diag;  // [N] diagonal rank in the scalar row
  const uint8_t* cslot_diag;   // [N] slot of the diagonal in the coupled-matrix ELL
  float2* cval_a; // [r*ld + i] {A_uu (=A_vv), A_pp}
  float2* cval_g; // [r*ld + i] {A_up (=A_pu), A_vp (=A_pv)}
  float2* cdiag2; // [ld] {s_pu, s_pv} of the diagonal block
  float* sval;    // [r*ld + i] scalar pressure matrix
  float* rhs;     // [3N]
  float* dinv_uv; // [N]
  float* dinv_p;  // [N]
};

// The Krylov kernels process 4 consecutive rows per thread: every per-slot
// array is one 16/32-byte load per thread, columns are 16-bit deltas when the
// whole matrix allows it, lengths / diagonal ranks u8.
struct CoupledMatrix {
  uint32_t N;
  uint32_t r0, r1;        // rows this launch processes (multiples of 4 except r1 = N)
  uint32_t r2, r3;        // optional second row range of the same launch (empty: r3 <= r2)
  uint32_t ld;            // slot stride (N rounded up to 64)
  int ws;
  int use16;
  // aligned-slot ELL (Topology::tslot): entries of a row sit in increasing
  // slots (CSR order), gaps where a neighbour is missing
  const int32_t* col;     // [r*ld + i] signed local column (gaps: a virtual column)
  const int16_t* col16;   // [r*ld + i] col - i (use16)
  const uint16_t* lg;     // [ld] slots in use (bits 0-6) | regular row (bit 7) | gap mask << 8
  const uint8_t* drank;   // [ld] slot of the diagonal
  const float2* cval_a;
  const float2* cval_g;
  const float2* cdiag2;   // [ld]
  // regular rows (lg bit 7): every slot's column is row + tmode[slot] (the
  // per-slot modal delta), so the kernels derive the columns instead of
  // loading them; set when ws <= kCoupledRegMaxWs (one peeled slot group)
  int reg;
  int tmode[8];
};
constexpr uint32_t kLgUsedMask = 0x7Fu, kLgRegular = 0x80u;
constexpr int kCoupledRegMaxWs = 5;

// One AMG level (linear_solver/amg.rs AmgLevel) in the layout the gfx950
// kernels stream: off-diagonal entries only, ELL slot-major with row stride
// `stride` (= n rounded up to 64, so four consecutive rows of one slot are one
// 16-byte load), columns as 16-bit deltas (col - row) when every delta of the
// level fits, else 32-bit; per-row length and diagonal position as u8.
// Off-diagonals keep the reference CSR order (ascending column), so every
// row sum accumulates in the reference order.
struct AmgLevelDev {
  uint32_t n;
  uint32_t r0, r1;       // rows a smoother / residual launch processes (default 0, n)
  uint32_t r2, r3;       // optional second row range of the same launch (empty: r3 <= r2)
  uint32_t stride;       // row stride of the ELL slots (n rounded up to 64)
  int w;                 // ELL width (max off-diagonals per row)
  int use16;             // 1: col16 holds deltas; 0: col32 holds absolute columns
  int full;              // slot-load mode of the row kernels (amg_rows.hpp gather_group): 0 or 1
  const float* val;      // [r*stride + i]
  const int16_t* col16;  // [r*stride + i]  col - i
  const int32_t* col32;  // [r*stride + i] signed local column
  const uint8_t* len;    // [stride] off-diagonal count per row
  const uint8_t* drank;  // [stride] position of the diagonal among the row's entries
  const float* dv;       // [stride] raw diagonal value (0 if absent)
  const float* de;       // [stride] smoother diagonal (dv, or 1.0 if |dv| < 1e-14)
  // wide level (a row with more off-diagonals than kAmgWideLimit): 16-bit row
  // lengths / diagonal ranks here (len / drank then hold min(., 255) and are
  // not read).  Only the one-workgroup tail kernels run wide levels
  // (Solver::ensure_amg moves the tail up to the first wide level).
  const uint16_t* len16;
  const uint16_t* drank16;
  // coarsening operators (only when nc > 0)
  uint32_t nc;
  const uint32_t* agg;     // [stride] P: fine -> coarse (padding rows -> 0, never read)
  const uint32_t* r_row;   // [nc+1] R = P^T rows (fine indices ascending)
  const uint32_t* r_col;
  // [nc] the first 4 members of each aggregate (k_amg_restrict: one 16-byte
  // load instead of r_row -> r_col); -1 pads, r_m4[I].w < -1 flags an
  // aggregate with more than 4 members (the rest read through r_row / r_col)
  const int4* r_m4;
  // k_amg_resrestrict: aggregates per block (0: the level keeps the separate
  // residual + restriction kernels); every block's members fit kRRCap
  uint32_t rr_agg;
};
constexpr uint32_t kRRCap = 2048;  // residuals per block of k_amg_resrestrict (LDS floats)

// k_amg_resrestrict_pair: the down-leg of two adjacent single-GPU / replicated
// levels (i, i+1) in one launch.  A block owns level-(i+2) aggregates
// [jb[k], jb[k+1]); its level-(i+1) rows S = the members of those aggregates
// (R order, written by the block) then their off-diagonal columns outside
// them (the ring, recomputed redundantly); f lists the level-i members of every
// S row (R order).  Built at AMG setup (Solver::build_rr_pairs) so that every
// block's S, f and aggregates fit kPairThreads.
constexpr uint32_t kPairThreads = 1024;
constexpr int kPairW = 8;  // level-(i+1) slots prefetched before the level-i phase
struct AmgPairImage {
  uint32_t nblocks;
  uint32_t threads;    // block size = per-block capacity (256 or kPairThreads)
  const uint32_t* jb;  // [nblocks + 1] level-(i+2) aggregate ranges
  const uint32_t* sb;  // [nblocks + 1] ranges in s
  const uint32_t* s;   // level-(i+1) rows: each block's members first, then its ring
  const uint32_t* fo;  // [|s| + 1] ranges in f of each s row's level-i members
  const uint32_t* f;   // level-i rows
  const uint16_t* lc;  // [r * stride_{i+1} + row] block-local index (in s) of slot r's column
};

// k_amg_prolong_smooth_pair: the up-leg of two adjacent single-GPU /
// replicated levels in one launch -- the post-smoother of coarse level c (its
// prolongation from c+1 applied to its reads, k_amg_smooth<..., PRO>) for the
// rows T the block needs, kept in LDS, then the post-smoother of fine level
// c-1 reading x_f + P x_c.  A block owns kUpPairRows consecutive fine rows;
// level c's smoothed x is never stored (nothing reads it after the up-leg).
constexpr uint32_t kUpPairRows = 256;
constexpr uint32_t kUpPairCap = 1024;  // T rows per block (LDS floats)
struct AmgUpPairImage {
  uint32_t nblocks;
  const uint32_t* tb;   // [nblocks + 1] ranges in t
  const uint32_t* t;    // level-c rows of each block (ascending)
  const uint16_t* lt;   // [r * stride_f + row] T-local index of agg_f[col] of fine slot r
  const uint16_t* lto;  // [stride_f] T-local index of agg_f[row]
};
// zeroed entries after every level's agg array: the fused prolongation reads
// agg with 16-byte loads from any column (as the x gathers, whose vectors
// carry the same slack)
constexpr size_t kAggSlack = 64;

// Halo pack (distributed): up to 8 fields packed per launch.
struct PackField {
  const float* src;   // owned-base pointer of the field
  int comps;          // floats per cell
  uint32_t stage_off; // offset of this field's block in the stage buffer (floats)
};
struct PackArgs {
  PackField f[8];
  int nf;
  const int32_t* idx;  // [n] owned local rows to send
  uint32_t n;
  float* stage;
};

// r_m4 image of R (amg.hip k_amg_restrict; built on the host, amg_device.cpp)
void build_r_m4(const std::vector<uint32_t>& r_row, const std::vector<uint32_t>& r_col, std::vector<int32_t>& out);

// Levels handled by the single-workgroup V-cycle tail kernel.
struct AmgTailLevel {
  AmgLevelDev L;
  float* x;
  float* xt;
  float* b;
  float* r;
};
constexpr int kMaxAmgLevels = 20;

// One tail level inside the LDS blob of k_amg_tail_blob (offsets in 32-bit
// words from the blob start, each array 16-byte aligned): off-diagonal CSR
// with u16 columns, diagonal data, P (agg, u16) and R (u16 CSR).
struct TailBlobLevel {
  uint32_t n, nc;
  uint32_t de, dv, rowoff, drank, val, col, agg, r_row, r_col;
  uint32_t maxlen;  // longest row (off-diagonal entries)
};

// ---------------- launch wrappers (one .hip per solver stage) ----------------
// ---- flux.hip ----
void launch_prepare(const PrepareArgs& a, hipStream_t s);
// test mode (reference semantics): the reference's racy prepare with its 64-cell
// workgroups in order, d_p / grad_p in place (a.dp_out / a.gp_out = a.st's),
// then every non-owner face slot e takes -flux_s[mirror[e]] (mirror[e] < 0:
// owner or boundary slot, kept)
void launch_prepare_ordered(const PrepareArgs& a, const int32_t* mirror, uint32_t slots, hipStream_t s);
void launch_assemble(const AssembleArgs& a, hipStream_t s);
// Boussinesq buoyancy (include/cfd2_amd.h "Arithmetic of buoyancy" is the
// contract), a second kernel argument of the buoyant assembly only: the plain
// kernel keeps its arguments.  f[0 .. n): the driving fields (beta != 0) in
// ascending field order; per owned cell, after the face loop and before the
// stores, one coalesced 4-byte load per entry:
//   d = phi[i] - ref;  fb = (vol_i * density) * (beta * d)
//   rhs_u = rhs_u - fb * gx;  rhs_v = rhs_v - fb * gy
// The matrix, rhs_p and the diagonal inverses keep the plain kernel's bits.
constexpr int kMaxBuoyancyFields = 4;
struct BuoyancyField {
  const float* phi;  // [N] the field as it stands at the launch
  float beta;
  float ref;
};
struct BuoyancyArgs {
  BuoyancyField f[kMaxBuoyancyFields];
  int32_t n;  // entries in use
  float gx, gy;
};
void launch_assemble_buoyant(const AssembleArgs& a, const BuoyancyArgs& b, hipStream_t s);
// Prescribed boundary velocities (include/cfd2_amd.h "Arithmetic of boundary
// velocities" is the contract), one more kernel argument of the BCV forms only:
// the plain kernels keep their arguments.  sel[i] = 0: cell i has no selected
// slot; else 1 + its row in the compact table, tab[row * fs.wf + k] = {bx, by,
// kind, 0} of slot k: kind 0 not selected, 1 a selected inlet slot, 3 a selected
// wall slot (the slot's boundary type as a float).  The table has one row per
// cell with a selected slot, O(sqrt N) rows; it is read only inside the branch
// of a boundary slot of such a cell.  Per selected slot
//   g = scale * ramp (scale: inlet_scale on an inlet slot, wall_scale on a wall slot)
//   ubx = bx * g;  uby = by * g
// replace inlet_velocity * ramp, 0 (inlet) and 0, 0 (wall).
struct BcvArgs {
  const uint32_t* sel;  // [N]
  const float4* tab;    // [rows * fs.wf]
  float inlet_scale, wall_scale;
};
constexpr float kBcvInlet = 1.0f, kBcvWall = 3.0f;
void launch_prepare_bcv(const PrepareArgs& a, const BcvArgs& v, hipStream_t s);
// buoy: null for the form without the Boussinesq source
void launch_assemble_bcv(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs& v, hipStream_t s);
// Variable viscosity (include/cfd2_amd.h "Arithmetic of variable viscosity" is
// the contract), one more kernel argument of the VISC forms only: mu [N], the
// viscosity per cell as it stands at the launch.  Per face slot of cell i, one
// f32 rounding per operation,
//   interior  mu_f = 0.5f * (mu[i] + mu[other])   (the same bits from either side)
//   boundary  mu_f = mu[i]
// and mu_f stands where c.viscosity stood: diff_coeff = mu_f * area / dist with
// the kernel's own distance (dist_e in prepare, dist_a in assemble).  One more
// coalesced 4-byte load per cell and one 4-byte gather per interior slot.
// v / buoy: null for the forms without them.
void launch_prepare_visc(const PrepareArgs& a, const BcvArgs* v, const float* mu, hipStream_t s);
void launch_assemble_visc(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs* v, const float* mu,
                          hipStream_t s);
// Volume penalisation (include/cfd2_amd.h "Arithmetic of volume penalisation" is
// the contract), one more kernel argument of the PEN forms only: a linear drag
// towards a target velocity, diagonal and implicit.  Per cell i, all f32, one
// rounding per operation, uc = st.u[i] (the iterate both kernels already load):
//   s   = sigma[i]                                              forch null
//   s   = sigma[i] + forch[i] * sqrtf(uc.x*uc.x + uc.y*uc.y)    forch set
//   pen = vol[i] * s
//   prepare : diag_coeff += pen     after the face loop, before dp_new
//   assemble: diag_uv    += pen     after the face loop and the BUOY block
//             rhs_u += pen * (target_scale * target[i].x)       target set; null: nothing is added
//             rhs_v += pen * (target_scale * target[i].y)
// forch and target are tested as kernel arguments: uniform over the launch (as
// k_wall_motion tests mu).  One more coalesced 4-byte load per cell, 4 more with
// forch, 8 more with target; no gather.  The PEN forms are one templated
// __global__ per stage, every argument struct present and the unused ones
// empty; v / mu / buoy: null for the forms without them.
struct PenaltyArgs {
  const float* sigma;    // [N]
  const float* forch;    // [N] or null
  const float2* target;  // [N] or null
  float target_scale;
};
void launch_prepare_pen(const PrepareArgs& a, const BcvArgs* v, const float* mu, const PenaltyArgs& pn, hipStream_t s);
void launch_assemble_pen(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs* v, const float* mu,
                         const PenaltyArgs& pn, hipStream_t s);
// ---- penalty.hip ----
// Read-only diagnostic of the penalisation: the force of the fluid on the
// penalised medium, its torque about (x0, y0), the rate of work of that force on the moving medium and
// the number of penalised cells, over the cells whose f64 centre ctr[i] lies in
// the closed box (box_on; the force region's rule: none for x1 < x0).  Per cell,
// in f64, every f32 value widened first, one rounding per operation:
//   s  = sigma (+ forch * sqrt(ux*ux + uy*uy))      forch set
//   m  = vol * s;  tx = scale * target.x, ty = scale * target.y   (0, 0 with target null)
//   fx = m * (ux - tx);  fy = m * (uy - ty)
//   sums: fx, fy, rx * fy - ry * fx (r = ctr[i] - (x0, y0)), fx * tx + fy * ty, s > 0 ? 1 : 0
// Unit partials partial[c * np + unit] in the canonical tree.
constexpr int kPenaltySums = 5;
struct PenaltyForceArgs {
  uint32_t N;
  const float* vol;
  const float2* u;
  PenaltyArgs pn;
  const double2* ctr;  // [N]
  double x0, y0;
  int32_t box_on;
  double box[4];       // x0, y0, x1, y1
  SumOut out;          // [kPenaltySums * np]
};
void launch_penalty_force(const PenaltyForceArgs& a, hipStream_t s);
// ---- viscosity.hip ----
// The viscosity models (include/cfd2_amd.h "Arithmetic of the viscosity
// models"): per cell the Green-Gauss gradients of u as prepare_cell forms them,
// the f32 shear rate, the model in f64 (pow_det.hpp), clamped, into mu and
// gdot.  stats[0..3]: min and max of mu as bit patterns, the cells clamped
// below and above; the caller sets them to {0xFFFFFFFF, 0, 0, 0} before the
// launch.  v != null: the face values of the BCV form.
struct ViscosityModelArgs {
  uint32_t N;
  cfd_constants c;
  FaceSlots fs;
  const float* vol;
  const float2* u;
  cfd_viscosity_model model;
  float* mu;        // [N] out
  float* gdot;      // [N] out
  uint32_t* stats;  // [4]
};
void launch_viscosity_model(const ViscosityModelArgs& a, const BcvArgs* v, hipStream_t s);
// writes per-block max bit patterns to blockmax[2*nb] and the final pair to maxbits[0..1]
// (and to host_out[0..1], a device view of pinned host memory, when non-null)
void launch_update_fields(uint32_t N, float alpha_u, float alpha_p, const float* x, float2* u,
                          float* p, uint32_t* blockmax, uint32_t* maxbits, uint32_t* host_out, hipStream_t s);
// ---- krylov.hip ----
// unit partials (U chunks of 256 cells each) of dot(x, y) over 3-component cells
void launch_dot_partial(const float* x, const float* y, uint32_t N, uint32_t U, float* partial, hipStream_t s);
// Reference reduction order (test mode): partial[g] = the 64-wide halving tree
// of v[i] * v[i] over DOFs i in [64 g, 64 g + 64) of the 3N (norm_sq_partial,
// gmres_ops.wgsl:195-223); ng = ceil(n3 / 64) groups
void launch_ref_norm_partials(const float* v, uint32_t n3, float* partial, hipStream_t s);
// partial[ii * pstride + g] = the same tree of V_ii[i] * w[i], V_ii = binv[ii] *
// W_ii, ii = 0..j (calc_dots_cgs, gmres_cgs.wgsl:28-82)
void launch_ref_cgs_dots(const float* w, const float* basis, const float* binv, size_t stride, int j, uint32_t n3,
                         float* partial, uint32_t pstride, hipStream_t s);
// total of the reduction r (one vector): mode 1: out[0] = sqrt(total); mode 2:
// also *inv = 1.0f / sqrt (host-style) and g0 (if non-null) = sqrt
// g0 (mode 2): g0[0] = norm, g0[1..g_len) = 0; host_out (device view of pinned host memory, or null) = norm
void launch_reduce_final(const RedSrc& r, int mode, float* out, float* inv, float* g0, int g_len, float* host_out,
                         hipStream_t s);
// ---- coupled_rows.hip ----
// b != null: y = b - A x with the residual axpby's operations (1 * b + -1 * (A x))
// nt: the matrix and b are read with the nontemporal policy (device_util.hpp ldx)
void launch_spmv(const CoupledMatrix& A, const float* x, float* y, hipStream_t s, const float* b = nullptr,
                 bool nt = false);
// ---- krylov.hip ----
// basis: unnormalised W_i at basis + i*stride, scales binv[i]; unit partials
// partial[ii * np + k] of <w, V_ii>, ii = 0..j
// keep_bytes > 0: the last blocks (their j + 2 vectors within keep_bytes) read
// the basis with the default policy, for a top-down update (rev) after it
void launch_cgs_dots(const float* w, const float* basis, const float* binv, size_t stride, int j,
                     uint32_t N, uint32_t U, float* partial, uint32_t np, hipStream_t s, size_t keep_bytes = 0,
                     bool lat = false);
// H[j][ii] = total of vector ii of r (r.nvec = j + 1)
void launch_cgs_reduce(const RedSrc& r, int j, float* H, int m1, hipStream_t s);
// W_{j+1} = w - sum_i H[i,j] V_i  (written into basis slot j+1) + ||W_{j+1}||^2 unit partials
// fr != null: the CGS totals (H column j) reduced inside the update from the
// dots' unit partials (k_cgs_reduce not launched); only where
// cgs_reduce_fusable(*fr) holds -- one GPU, at most 256 padded units
void launch_cgs_update_norm(const float* w, float* basis, const float* binv, size_t stride, int j, float* H,
                            int m1, uint32_t N, uint32_t U, float* partial, hipStream_t s, bool rev = false,
                            bool ntb = true, const RedSrc* fr = nullptr, bool lat = false);
// small meshes (<= CFD_CGS_LAT_MAX_CELLS): the CGS dots / update in their
// latency form (several basis vectors per load round trip; same bits)
bool cgs_latency_form(uint32_t N);
// large meshes (>= CFD_CGS_SER_MIN_CELLS): the CGS kernels keep one basis load in flight per wavefront
bool cgs_serial_form(uint32_t N);
bool cgs_reduce_fusable(const RedSrc& r);
// ||W_{j+1}|| = sqrt(total of r) -> H[j+1,j], binv[j+1]; Givens update of column j; resid_hist[j] = |g[j+1]|,
// also into host_resid[j] (device view of pinned host memory) when non-null
void launch_norm_givens(const RedSrc& r, int j, float* H, int m1, float* givens, float* g, float* binv,
                        float* resid_hist, float* host_resid, hipStream_t s);
// ---- coupled_rows.hip ----
// r_in = binv[j] * W_j
void launch_precond_predict(const CoupledMatrix& A, const float* w_in, const float* binv, int j,
                            const float* dinv_uv, const float* dinv_p, float* temp_p, float* p_sol,
                            float* p_prev, hipStream_t s, bool nt = false);
// one relax_pressure sweep, 4 rows per thread over the scalar ELL image viewed as
// an AmgLevelDev (val = the live scalar matrix, len / col16 / col32 incl. the
// diagonal, skipped by `drank`); rows [L.r0, L.r1) + [L.r2, L.r3)
void launch_relax_pressure4(const AmgLevelDev& L, const uint8_t* drank, const float* dinv_p, const float* temp_p,
                            const float* src, float* dst, hipStream_t s);
// all `iters` relax_pressure sweeps in one single-workgroup launch (p_sol / temp
// ping-pong as the per-sweep launches, the final iterates back in both); false
// when N > kRelaxFusedMaxRows or the ELL width is too wide for the register image
constexpr uint32_t kRelaxFusedMaxRows = 8191;  // two (N + 1)-float iterates in 64 KiB of LDS
bool launch_relax_pressure_fused(uint32_t N, uint32_t ld, uint32_t ws, const int32_t* col, const uint32_t* len,
                                 const float* sval, const float* dinv_p, const float* temp_p, float* p_sol,
                                 float* temp, uint32_t iters, hipStream_t s);
void launch_precond_correct(const CoupledMatrix& A, const float* w_in, const float* binv, int j,
                            const float* p_sol, const float* dinv_uv, float* z, hipStream_t s);
// ---- krylov.hip ----
void launch_solve_triangular(const float* H, const float* g, float* y, int k, int m1,
                             hipStream_t s);
// lat: the latency form allowed (small meshes; false = the streaming form)
void launch_update_x(float* x, const float* z, size_t stride, const float* y, int k, size_t n,
                     hipStream_t s, bool lat = true);
// ---- amg.hip ----
// ev0/ev1 (optional): timing events recorded by the GPU at kernel start / end
// nt: the level matrix, b and the diagonal read with the nontemporal policy
void launch_amg_smooth(const AmgLevelDev& L, const float* x, const float* b, float* x_out,
                       hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, bool nt = false);
// post-smoother with the prolongation fused: x_out = smooth(x + P xc), bit-identical
// to launch_amg_prolong(L, x, xc) then launch_amg_smooth(L, x, b, x_out), but x is
// only read (single-GPU / replicated levels: every column an owned row)
void launch_amg_smooth_prolong(const AmgLevelDev& L, const float* x, const float* xc, const float* b,
                               float* x_out, hipStream_t s);
// test mode (reference semantics): the reference's in-place smoother with its
// 64-row workgroups run in order (rows of a workgroup read before any writes)
void launch_amg_smooth_ordered(const AmgLevelDev& L, float* x, const float* b, hipStream_t s);
// pre-smoother of a level whose x is identically +0 (bit-identical to launch_amg_smooth then)
void launch_amg_smooth_zero(const AmgLevelDev& L, const float* b, float* x_out, hipStream_t s);
void launch_amg_residual(const AmgLevelDev& L, const float* x, const float* b, float* r,
                         hipStream_t s, bool nt = false);
// coarse_b = R r and coarse_x = 0 (the reference's separate `clear` pass fused); on a
// distributed coarse level also clears its ghosts: [-glo, 0) and [stride_c, stride_c + ghi)
// sm_out != null: instead of clearing coarse_x, write the coarse level's
// zero-x pre-smoother result (mix(0, (b - 0)/de, 0.8), de = sm_de) to sm_out.
// Coarse rows [I0, I1) only (I1 = 0: all L.nc); `ghosts` false: no ghost
// clearing (a distributed launch split around the residual halo).
void launch_amg_restrict(const AmgLevelDev& L, const float* r, float* coarse_b, float* coarse_x,
                         uint32_t stride_c, uint32_t glo, uint32_t ghi, hipStream_t s,
                         float* sm_out = nullptr, const float* sm_de = nullptr, uint32_t I0 = 0,
                         uint32_t I1 = 0, bool ghosts = true);
// ---- amg_tail.hip ----
// V-cycle restricted to levels [first, nlev) of `tail` (device array), one workgroup:
// pre-smooth / residual / restrict+clear down, 10 coarsest sweeps, prolong / post-smooth up.
// Every level's x ends in tail[l].x (even sweep counts).
// lds_bytes > 0: the LDS-resident version (needs every tail vector in <= kTailLdsMax bytes)
constexpr size_t kTailLdsMax = 160 * 1024 - 1024;
void launch_amg_tail(const AmgTailLevel* tail, int first, int nlev, size_t lds_bytes, hipStream_t s);
// The LDS tail with the matrices in LDS too: `blob` (blob_words 32-bit words,
// a multiple of 4) is copied into LDS after the vectors (vec_floats floats);
// desc[l] describes level l (l in [first, nlev)).  lds_bytes = 4 * (vec_floats + blob_words).
void launch_amg_tail_blob(const AmgTailLevel* tail, const TailBlobLevel* desc, const uint32_t* blob,
                          uint32_t blob_words, uint32_t vec_floats, int first, int nlev, const float* b_first,
                          uint32_t n_first, hipStream_t s);
// ---- amg.hip ----
// fine rows [f0, f1) (multiples of 4 but f1 = L.n; f1 = 0: all)
// residual + restriction fused (k_amg_resrestrict; L.rr_agg > 0, replicated
// or single-GPU level): coarse_b = R (b - A x), coarse_x cleared or the
// coarse zero-x pre-smoother written to sm_out (as launch_amg_restrict)
void launch_amg_resrestrict(const AmgLevelDev& L, const float* x, const float* b, float* coarse_b, float* coarse_x,
                            float* sm_out, const float* sm_de, hipStream_t s);
// levels i (Lf: x, b) and i+1 (Lm) down-leg in one launch: writes level
// i+1's rhs bm and pre-smoothed x xm (as k_amg_resrestrict with sm_out), then
// level i+2's rhs cb and either its pre-smoothed x (sm_out, diagonal sm_de)
// or cx = 0 -- the bits of the two k_amg_resrestrict launches
// levels c (Lc: x xc, b bc; coarse x xcc of level c+1) and c-1 (Lf: x xf, b
// bf): writes only the fine level's post-smoothed x into xf_out -- the bits of
// the two k_amg_smooth<..., PRO> launches for the fine level
void launch_amg_prolong_smooth_pair(const AmgLevelDev& Lf, const AmgLevelDev& Lc, const AmgUpPairImage& P,
                                    const float* xf, const float* bf, float* xf_out, const float* xc,
                                    const float* bc, const float* xcc, hipStream_t s);
void launch_amg_resrestrict_pair(const AmgLevelDev& Lf, const AmgLevelDev& Lm, const AmgPairImage& P,
                                 const float* x, const float* b, float* bm, float* xm, float* cb, float* cx,
                                 float* sm_out, const float* sm_de, hipStream_t s);
void launch_amg_prolong(const AmgLevelDev& L, float* x, const float* coarse_x, hipStream_t s, uint32_t f0 = 0,
                        uint32_t f1 = 0, bool nt = false);
// ---- amg_tail.hip ----
// Sets the tail kernels' dynamic-LDS attribute on `device` (once per device,
// thread-safe; throws on failure) and returns their LDS budget there:
// min(kTailLdsMax, the device's opt-in per-block LDS).  Call with `device` current.
size_t init_kernel_attributes(int device);
// ---- stats_dist.hip ----
// check_evolution (coupled_solver.rs:501-580) statistics in the canonical order (f64):
// chunk partials partial[f * np + k], f = {evolution, sum_u, sum_v, sumsq_u, sumsq_v}
// The variance part reads record ((gbase + c) >> 2) - rec0 of `var` (stride bug, §0.1-12).
void launch_evolution_partial(StateView cur, StateView prev, int have_prev, uint32_t N,
                              StateView var, uint64_t gbase, uint64_t rec0, uint32_t U, double* partial, uint32_t np,
                              hipStream_t s);
// distributed helpers
void launch_pack(const PackArgs& a, hipStream_t s);
// distributed: this rank's segment values out[v * maxseg + s] of nvec reductions
// from their unit partials part[v * np + k] (k < nunits local, G units per segment)
void launch_seg_reduce(const float* part, uint32_t np, uint32_t nchunks, uint32_t G, int nvec, float* out,
                       uint32_t maxseg, hipStream_t s);
void launch_seg_reduce_d(const double* part, uint32_t np, uint32_t nchunks, uint32_t G, int nvec, double* out,
                         uint32_t maxseg, hipStream_t s);
void launch_max_combine(const uint32_t* gathered, int R, uint32_t* out, uint32_t* host_out, hipStream_t s);
// out[f] = total of vector f of r, f < r.nvec (check_evolution: 5 sums; flow diagnostics: 6)
void launch_evolution_final(const RedSrcD& r, double* out, hipStream_t s);

// ---- diagnostics.hip: flow diagnostics ----
// One read-only sweep over the owned cells of a state: Green-Gauss gradients of
// u as k_prepare forms them (the same bits), omega = dv/dx - du/dy and div =
// du/dx + dv/dy per cell, and per cell the f64 terms (each evaluated left to
// right from the f32 values)
//   0 kinetic energy 0.5 vol s, s = (double)u u + (double)v v
//   1 enstrophy      0.5 vol omega omega
//   2, 3 pressure force  sum over the selected wall slots of p n_x area, p n_y area
//   4, 5 viscous force   ... of viscosity u area / dist_e, viscosity v area / dist_e
// as unit partials partial[f * np + k] of the canonical tree, plus the maxima
// of s, |omega|, |div| as bit patterns (a NaN never becomes the maximum).
constexpr int kFlowDiagSums = 6;
struct FlowDiagArgs {
  uint32_t N;
  cfd_constants c;
  FaceSlots fs;
  const float* vol;
  const float2* u;            // owned base; neighbours through fs.other (ghosts current)
  const float* p;
  const uint16_t* wall_mask;  // [N] bit k: wall slot k is in the force region; null: no region (forces +0)
  float* omega_out;           // [N] or null (both null: the scalar-only pass)
  float* div_out;
  SumOut out;                 // [kFlowDiagSums * np]
  unsigned long long* blockmax;  // [3 * red_blocks(N)] scratch
};
// maxout[0..2] = bits of max s (f64), max |omega|, max |div| (f32 bits, zero-extended)
// v != null, the BCV form (BcvArgs above): the face value of a selected inlet or
// wall slot is (ubx, uby), and the viscous force of a selected wall slot in the
// force region is viscosity * ((double)u - (double)ubx) * area / dist_e.
// mu != null, the VISC form: (double)mu[i] for the viscosity of cell i's wall slots.
void launch_flow_diag(const FlowDiagArgs& a, const BcvArgs* v, const float* mu, unsigned long long* maxout,
                      hipStream_t s);
// Read-only wall-motion sums over the force-region wall slots (wall_mask, as
// FlowDiagArgs): per cell, in f64, in ascending slot order, with F_p = p n area
// and F_v = viscosity (u - ub) area / dist_e as k_flow_diag forms them and the
// lever arm r = ctr[row * fs.wf + k] - (x0, y0) (crow[i] = 1 + row, the compact
// table of the f64 face centres of the region's cells):
//   0 torque of F_p: r_x F_py - r_y F_px      1 torque of F_v
//   2 power: -((F_px + F_vx) ubx + (F_py + F_vy) uby) on a selected slot, else +0
// Unit partials partial[f * np + unit] in the canonical tree.  v.sel null: no
// selection (ub = 0 everywhere).
constexpr int kWallMotionSums = 3;
struct WallMotionArgs {
  uint32_t N;
  cfd_constants c;
  FaceSlots fs;
  const float2* u;
  const float* p;
  const uint16_t* wall_mask;  // [N]
  const uint32_t* crow;       // [N]
  const double2* ctr;         // [rows * fs.wf]
  BcvArgs v;
  const float* mu;            // [N] the viscosity per cell, or null: c.viscosity
  double x0, y0;
  SumOut out;                 // [kWallMotionSums * np]
};
void launch_wall_motion(const WallMotionArgs& a, hipStream_t s);

// ---- scalar.hip ----
// Passive scalar transport (include/cfd2_amd.h, the last section): implicit
// Euler, bounded first-order upwind, driven by the face-slot mass fluxes flux_s
// of the last k_prepare.  All f32, every sum left to right in face-slot order.
// Per owned cell i and slot k (e = k*N + i):
//   a_t    = vol_i * density / dt
//   diff_k = (density * D) * area_e / dist_e_e           (this order)
//   cin_k  = flux_s_e < 0 ? -flux_s_e : 0                (= max(-F, 0))
//   c_k    = cin_k + diff_k   internal and inlet slots;  0 wall and outlet slots
//   diag_i = a_t + c_0 + c_1 + ...
//   b_i    = a_t * phi_old_i, then + c_k * inlet_value per inlet slot
// coef is slot-major with row stride ld (N rounded up to 64): coef[k*ld + i].
struct ScalarAssembleArgs {
  uint32_t N;
  uint32_t ld;
  FaceSlots fs;
  const float* vol;
  const float* flux_s;   // [k*N + i]
  const float* phi_old;  // [N]
  float density, dt, diffusivity, inlet_value;
  float* coef;           // [k*ld + i], k < nface_i written
  float* diag;           // [N]
  float* b;              // [N]
};
void launch_scalar_assemble(const ScalarAssembleArgs& a, hipStream_t s);
// Scheme 1, "limited linear" (include/cfd2_amd.h "Arithmetic of scheme 1" is
// the contract): the Green-Gauss gradient of phi_old with the face values of
// prepare_cell's vfu branch, then the assembly above with b_i = the clamped
// a_t * phi_old_i - corr_i (+ the inlet terms).  coef and diag get the bits
// launch_scalar_assemble writes.
struct ScalarGradArgs {
  uint32_t N;
  FaceSlots fs;
  const float* vol;
  const float* phi_old;  // [N]
  float inlet_value;
  float2* g;             // [N]
  // the field the assembly `a` is for
  ScalarGradArgs(const ScalarAssembleArgs& a, float2* g_)
      : N(a.N), fs(a.fs), vol(a.vol), phi_old(a.phi_old), inlet_value(a.inlet_value), g(g_) {}
};
void launch_scalar_grad(const ScalarGradArgs& a, hipStream_t s);
struct ScalarLimitedArgs {
  ScalarAssembleArgs a;
  const float2* g;    // [N] launch_scalar_grad's, complete before this launch
  uint32_t* clamped;  // one word: += the cells whose t the clamp changed (the caller zeroes it)
};
void launch_scalar_assemble_limited(const ScalarLimitedArgs& a, hipStream_t s);
// Wall conditions and sources of one field (include/cfd2_amd.h "Arithmetic of
// wall conditions and sources" is the contract), a second kernel argument of
// the boundary-condition forms only: the plain kernels above keep their
// arguments.  sel[i]: bit k < 31 = slot k of cell i is a selected wall slot, bit
// 31 = cell i is a source cell (the host builds it; a bit is set on wall slots
// only).  Per selected wall slot, at the slot's place in the loop:
//   kind 1   c_k = (density * D) * area / dist_e;  diag += c_k;  b += c_k * value
//   kind 2   c_k = 0;  b += value * area
// and after the slot loop b += vol_i * rate in a source cell.  Scheme 1: the
// gradient's face value and the clamp's range take `value` on a kind-1 slot; the
// inlet, kind-1 and kind-2 terms follow the clamp in one pass in slot order.
struct ScalarBC {
  const uint32_t* sel;  // [N]
  int32_t kind;         // 0 (sources only), 1 fixed value, 2 fixed flux
  float value;
  float rate;           // 0: bit 31 of sel is clear everywhere
};
void launch_scalar_assemble_bc(const ScalarAssembleArgs& a, const ScalarBC& bc, hipStream_t s);
void launch_scalar_grad_bc(const ScalarGradArgs& a, const ScalarBC& bc, hipStream_t s);  // kind 1 only
void launch_scalar_assemble_limited_bc(const ScalarLimitedArgs& a, const ScalarBC& bc, hipStream_t s);
// Read-only wall-flux diagnostic of one field: per cell, in f64 in slot order
// over its selected slots, flux (kind 1: (double)c_k * ((double)value -
// (double)phi_i), c_k the f32 above; kind 2: (double)value * (double)area), area
// and area * phi_i; a cell without a selected slot reads none of its slot
// arrays and adds +0.  Unit partials partial[f * np + unit], f = 0 flux, 1 area,
// 2 phi_area, in the canonical tree (as launch_scalar_stats writes its sum).
constexpr int kWallFluxSums = 3;
struct ScalarWallFluxArgs {
  uint32_t N;
  const float* area;     // fs.area, [k*N + i]
  const float* dist_e;   // fs.dist_e
  const uint32_t* sel;   // [N]
  const float* phi;      // [N]
  float rd;              // density * D
  int32_t kind;          // 1 or 2
  float value;
  SumOut out;            // [kWallFluxSums * np]
};
void launch_scalar_wall_flux(const ScalarWallFluxArgs& a, hipStream_t s);
// Read-only body-force diagnostic of the buoyancy the assembly adds (flux.hip
// BuoyancyArgs), the counterpart of k_flow_diag's wall force: per cell, in f64,
// from +0 over the driving fields in field order,
//   m = (((double)vol_i * (double)density) * (double)beta) * ((double)phi_i - (double)ref)
//   t_x = t_x - m * (double)gx;  t_y = t_y - m * (double)gy
// Unit partials partial[c * np + unit], c = 0 x, 1 y, in the canonical tree (as
// launch_scalar_stats writes its sum).
constexpr int kBuoyancySums = 2;
struct BuoyancyForceArgs {
  uint32_t N;
  const float* vol;
  BuoyancyArgs b;
  float density;
  SumOut out;  // [kBuoyancySums * np]
};
void launch_buoyancy_force(const BuoyancyForceArgs& a, hipStream_t s);
// The assembled system as the solvers read it: the Jacobi row of cell i is
//   J(phi)_i = (b_i + sum over internal slots k of c_k * phi[other_k]) / diag_i,
// the sum left to right in slot order (boundary slots skipped), a true
// division.  The columns are fs.other as it stands (stride N).  It leads both
// solvers' argument blocks, so its scalars and pointers are the kernel
// arguments preloaded into SGPRs.
struct ScalarSystem {
  uint32_t N;
  uint32_t ld;
  const int32_t* other;   // fs.other
  const uint32_t* nface;  // fs.nface
  const float* coef;
  const float* diag;
  const float* b;
};
// One Jacobi sweep: phi_out = J(phi_in), the sum starting from b_i.
struct ScalarSweepArgs {
  ScalarSystem sys;
  const float* phi_in;
  float* phi_out;
  uint32_t* blockmax;     // [scalar_sweep_blocks(N)] scratch of the delta form
};
uint32_t scalar_sweep_blocks(uint32_t N);
// What the sweep and the statistics leave for the host, one device object.
struct ScalarResults {
  uint32_t delta, pad;  // launch_scalar_sweep
  uint32_t kmin, kmax;  // launch_scalar_stats
  double integral;      // launch_evolution_final over the statistics' partials
};
static_assert(offsetof(ScalarResults, delta) == 0 && offsetof(ScalarResults, kmin) == 8 &&
                  offsetof(ScalarResults, kmax) == 12 && offsetof(ScalarResults, integral) == 16,
              "ScalarResults: the words the kernels write");
// delta != null: the sweep also leaves delta[0] = bits of max_i |phi_out_i -
// phi_in_i| (non-negative f32 values order as unsigned integers; a NaN
// difference counts as +inf, 0x7f800000, so it never reads as converged)
void launch_scalar_sweep(const ScalarSweepArgs& a, uint32_t* delta, hipStream_t s);
// Read-only statistics of one field: unit partials partial[k] (k < np) of
// sum (double)vol_i * (double)phi_i in the canonical tree (as k_flow_diag
// writes its sums), and res->kmin, res->kmax = min and max of phi as
// order-preserving keys (scalar_key_value decodes them; NaN cells are ignored,
// no cell: NaN).
struct ScalarStatsArgs {
  uint32_t N;
  const float* vol;
  const float* phi;
  SumOut out;          // [np]
  uint32_t* blockmm;   // [2 * red_blocks(N)] scratch
};
void launch_scalar_stats(const ScalarStatsArgs& a, ScalarResults* res, hipStream_t s);
// BiCGStab on the Jacobi-scaled system of the assembled field (include/
// cfd2_amd.h "Arithmetic of method 1" is the contract).  The operator and the
// x / r update run over blocks of 4 chunks (kRedBlockCells, as k_scalar_stats)
// and leave the unit partials of their dots in partial[v * np + unit] and the
// block maxima of |r| in blockmax; one-block finishing kernels turn them into
// the coefficients and the status words.  Everything after a stop returns at
// once: x is frozen.
constexpr uint32_t kKryDone = 0, kKryReason = 1, kKryIter = 2, kKryRes = 3, kKryMode = 4;  // state words
// The solver's device state, one object; the finishing kernels write it, the
// host reads st[0..3] once per batch.
struct ScalarKrylovState {
  double dv[4];    // rho, alpha, omega in f64
  uint32_t st[8];  // done, reason, iteration, bits of max |r|, mode of the x / r update
  float co[4];     // alpha, omega, beta rounded to f32
};
static_assert(offsetof(ScalarKrylovState, dv) == 0 && offsetof(ScalarKrylovState, st) == 32 &&
                  offsetof(ScalarKrylovState, co) == 64,
              "ScalarKrylovState: the words the kernels write");
struct ScalarKrylovArgs {
  ScalarSystem sys;
  float* x;               // [N] phi_old on entry, the frozen iterate after the stop
  float *rh, *r, *p, *v, *s, *t;  // [N] work vectors
  SumOut out;             // [2 * np]
  uint32_t* blockmax;     // [red_blocks(N)]
  ScalarKrylovState* state;
  RedSrcD red;           // combine(partial, 2)
  float tol;
};
// r = rh = p = J(x) - x, rho, max |r|; the state words (stop with reason 1 at
// iteration 0 if max |r| <= tol)
void launch_scalar_krylov_start(const ScalarKrylovArgs& a, hipStream_t s);
// iteration k (1-based) and, for k < max_iters, the beta and p of iteration k + 1
void launch_scalar_krylov_iteration(const ScalarKrylovArgs& a, uint32_t k, uint32_t max_iters, hipStream_t s);
// key of an f32 bit pattern: increasing in the value over every non-NaN float
__host__ __device__ inline uint32_t scalar_value_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__host__ __device__ inline uint32_t scalar_key_value(uint32_t key) { return (key & 0x80000000u) ? key & 0x7FFFFFFFu : ~key; }

// ---- render.hip ----
// A cell field as an RGBA8 image (include/cfd2_amd.h "The picture" is the
// contract): the ownership map of a view, built once, and per frame one thread
// per pixel.  All f32, nothing fused.
constexpr uint32_t kRenderNone = 0xFFFFFFFFu;
// Pixel boxes of at most this many pixels are tested by the cell's own thread;
// larger cells go to a list and get a wavefront each.  At 16 a thread's loop is
// at most 16 pixels x the fan, the same order as a face-slot loop (see DESIGN
// section 5.4 for what was measured).
constexpr uint32_t kRenderInPlacePixels = 16;
struct RenderPolys {
  uint32_t N;
  const float* vx;      // [num_vertices]
  const float* vy;
  const uint32_t* off;  // [N + 1]
  const uint32_t* idx;  // [off[N]], every entry < num_vertices
};
struct RenderView {
  uint32_t W, H;
  float x0, y1;  // the left and the top bound
  float dx, dy;
};
// The map while it is built holds owner + 1 (0: none), so that atomicMax
// yields the largest index; launch_render_map_finish turns it into owner /
// kRenderNone in place.  counts[0]: the cells listed, counts[1]: the owned
// pixels (the caller zeroes both and the map).
void launch_render_map_cells(const RenderPolys& p, const RenderView& v, uint32_t* map, uint32_t* list, uint32_t* counts,
                             hipStream_t s);
void launch_render_map_listed(const RenderPolys& p, const RenderView& v, uint32_t* map, const uint32_t* list,
                              uint32_t nlist, hipStream_t s);
void launch_render_map_finish(uint32_t* map, uint32_t npix, uint32_t* covered, hipStream_t s);
struct RenderValue {
  int32_t mode;     // 0 |u|, 1 u.x, 2 u.y, 3 f
  const float2* u;  // [N] modes 0..2
  const float* f;   // [N] mode 3
};
inline uint32_t render_range_blocks(uint32_t N) { return (N + 1023u) / 1024u; }
// keys[0], keys[1] = the minimum and the maximum of the value over the N cells
// as scalar_value_key keys, NaN cells ignored (none left: ~0 and 0).
// blockmm: [2 * render_range_blocks(N)] scratch.
void launch_render_range(const RenderValue& f, uint32_t N, uint32_t* blockmm, uint32_t* keys, hipStream_t s);
// One frame: rgba[q] = the packed pixel q (R in the low byte).  keys != null:
// the range is decoded from them (keys[0] > keys[1]: (0, 1)), else (lo, hi).
void launch_render_shade(const RenderValue& f, const uint32_t* map, uint32_t npix, const uint32_t* keys, float lo,
                         float hi, uint32_t* rgba, hipStream_t s);

// ---- particles.hip ----
// Tracer particles (include/cfd2_amd.h "The tracers" is the contract): located
// in the mesh through a bin grid, advanced face to face through the frozen
// piecewise-constant velocity, counted, stamped into a frame.  All f32, nothing
// fused; every kernel is one thread per particle, any count (block tails).
constexpr uint32_t kParticleSignBit = 0x80000000u;  // ParticleMesh::sa: g = -E
constexpr uint32_t kParticleCapped = 0x80000000u;   // ParticleSet::hops: the last advance hit the hop cap
constexpr uint32_t kParticleNoCell = 0xFFFFFFFFu;
struct ParticleMesh {
  uint32_t N;  // 0: no mesh
  int wf;
  const float* vx;      // [num_vertices]
  const float* vy;
  const uint32_t* off;  // [N + 1] the CCW polygons (locate)
  const uint32_t* idx;  // [off[N]]
  // the two vertices of every face slot, [k * N + c] like FaceSlots: sa the
  // smaller index, with kParticleSignBit set where the cell's polygon runs from
  // the larger index to the smaller one (g = -E); sb the larger index
  const uint32_t* sa;
  const uint32_t* sb;
  // the bin grid: nb x nb bins of (sx, sy) from (bx0, by0); bin (i, j)'s cells
  // are bin_cells[bin_off[j * nb + i] .. bin_off[j * nb + i + 1]), ascending
  uint32_t nb;
  float bx0, by0, sx, sy;
  const uint32_t* bin_off;
  const uint32_t* bin_cells;
};
// the bin of one coordinate (host and device: the listing and the lookup agree)
__host__ __device__ inline uint32_t particle_bin(float x, float x0, float s, uint32_t nb) {
  const float f = floorf((x - x0) / s);
  if (!(f >= 0.0f)) return 0u;  // also a NaN
  return f > (float)(nb - 1u) ? nb - 1u : (uint32_t)f;
}
struct ParticleSet {  // SoA, 4-byte fields, [capacity]
  uint32_t n;
  float* x;
  float* y;
  uint32_t* cell;
  uint32_t* status;
  float* age;
  uint32_t* contacts;
  uint32_t* hops;  // of the last advance | kParticleCapped
};
// Slots [first, first + count): position (x, y), age 0, no contacts, located.
void launch_particles_locate(const ParticleMesh& m, const ParticleSet& p, uint32_t first, uint32_t count, const float* x,
                             const float* y, hipStream_t s);
void launch_particles_advance(const ParticleMesh& m, const FaceSlots& fs, const float2* u, const ParticleSet& p, float dt,
                              uint32_t hop_cap, hipStream_t s);
// out[0..4] the slots per status, [5] wall contacts, [6] hops of the last
// advance, [7] their maximum over the particles, [8] particles that hit the
// cap.  The caller zeroes out.
constexpr int kParticleStats = 9;
void launch_particles_stats(const ParticleSet& p, unsigned long long* out, hipStream_t s);
void launch_particles_stamp(const ParticleSet& p, const RenderView& v, uint32_t colour, uint32_t* rgba, hipStream_t s);

// ---- timestats.hip ----
// Per-cell time statistics (include/cfd2_amd.h "Arithmetic of the time
// statistics" is the contract): one sample of weight w enters every enabled
// plane in one pass, all f64, nothing fused.  Planes, each [N] at stride ld
// (even: a lane's two cells are one 16-byte access): 0 m_u, 1 m_v, 2 m_p; with
// second moments 3 M_uu, 4 M_uv, 5 M_vv, 6 M_pp; then per field f its mean and
// M_ff, and with second moments M_uf and M_vf.
constexpr uint32_t kTimeStatsMaxFields = 4;
inline uint32_t tstats_planes(bool second_moments, uint32_t nf) {
  return 3u + (second_moments ? 4u : 0u) + nf * (second_moments ? 4u : 2u);
}
struct TimeStatsArgs {
  uint32_t N;
  uint32_t nf;            // fields, 0..kTimeStatsMaxFields
  const float2* u;        // [N] the current state
  const float* p;
  double* planes;
  size_t ld;
  double w, r;            // the sample's weight and w / (W + w), from the host
  const float* phi[kTimeStatsMaxFields];
};
void launch_tstats(const TimeStatsArgs& a, bool second_moments, hipStream_t s);
// One monitor sample: time_out[0..1] = time, dt; probe_out[t * (3 + ns) + ..] =
// u.x, u.y, p and the ns fields at cells[t]; diag_out (or null) = the nine words
// of the flow diagnostics' device result (diag_res: six f64 sums, three maxima).
constexpr uint32_t kMonitorDiagWords = 9;
struct MonitorRecordArgs {
  uint32_t P, ns;
  const uint32_t* cells;  // [P], every entry < N
  const float2* u;
  const float* p;
  const float* phi[kTimeStatsMaxFields];
  float time, dt;
  float* time_out;        // the slot's [2]
  float* probe_out;       // the slot's [P * (3 + ns)]
  const uint64_t* diag_res;
  uint64_t* diag_out;     // the slot's [kMonitorDiagWords], or null
};
void launch_monitor_record(const MonitorRecordArgs& a, hipStream_t s);

// ---- surface.hip ----
// Wall surface distributions (include/cfd2_amd.h "Arithmetic of the surface
// channels" is the contract): one thread per face of the compact table (cell,
// slot), all f64 from the f32 inputs, nothing fused.  Channels, each [n] at
// stride ld (n rounded up to 64): 0 p; 1, 2 the pressure force terms of
// k_flow_diag; 3, 4 its viscous terms (BCV form: relative to the wall's own
// velocity); then per field f its wall-flux term (k_scalar_wall_flux's t[0]
// term, +0 on a slot outside the field's wall selection) and phi_f of the cell.
// The plain form reads neither BcvArgs::sel nor the table.
constexpr uint32_t kSurfaceBaseChannels = 5;
inline uint32_t surface_channels(uint32_t nf) { return kSurfaceBaseChannels + 2u * nf; }
struct SurfaceField {
  const float* phi;     // [N]
  const uint32_t* sel;  // [N] the field's image word (ScalarBC), null: no wall selection
  float rd;             // density * D
  int32_t kind;         // 1 fixed value, 2 fixed flux (with sel)
  float value;
};
struct SurfaceArgs {
  uint32_t n;             // faces
  uint32_t N;             // cells: the slot arrays' row stride
  uint32_t nf;            // fields, 0..kTimeStatsMaxFields
  const uint32_t* cell;   // [n], every entry < N
  const uint32_t* slot;   // [n], every entry < wf
  cfd_constants c;
  const float2* u;
  const float* p;
  const float* area;      // fs.area, [k*N + i]
  const float* nx;
  const float* ny;
  const float* dist_e;
  uint32_t wf;            // the row width of BcvArgs::tab
  SurfaceField f[kTimeStatsMaxFields];
  size_t ld;
  double* out;            // sample: [channels * ld]
  double* mean;           // accumulate: [channels * ld] each
  double* m2;
  double w, r;            // accumulate: the sample's weight and w / (W + w), from the host
};
// v null: the plain form
void launch_surface_sample(const SurfaceArgs& a, const BcvArgs* v, const float* mu, hipStream_t s);
// the same evaluation, every channel into its mean and M2 (mean_update /
// m2_update of device_util.hpp) instead of a.out: one launch per sample
void launch_surface_accumulate(const SurfaceArgs& a, const BcvArgs* v, const float* mu, hipStream_t s);

}  // namespace cfd2
