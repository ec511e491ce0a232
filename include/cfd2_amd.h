/*
 * cfd2_amd.h — C ABI of the MI355X-native coupled incompressible-flow step.
 *
 * Drop-in boundary for the reference crate `cfd2` (TSultanov/cfd-demo2).
 * Every solver entry point replaces one method of the reference's
 * `impl GpuSolver` (Rust, src/solver/gpu/solver.rs / init/mod.rs); the Rust
 * extern "C" shim that binds them is in INTEGRATION.md.  Plain pointers and
 * sizes only; no torch types.  Calls are blocking and single-threaded per
 * handle, as in the reference (GpuSolver holds RefCells; GUI wraps it in a
 * Mutex).  Errors are returned as cfd_status (the reference panics instead);
 * cfd_last_error() gives a thread-local message.
 */
#ifndef CFD2_AMD_H
#define CFD2_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cfd_status {
  CFD_OK = 0,
  CFD_ERR_INVALID = 1,    /* bad argument / inconsistent mesh                    */
  CFD_ERR_HIP = 2,        /* HIP runtime failure (no device, OOM, launch error)  */
  CFD_ERR_DIVERGED = 3,   /* NaN residual: coupled_solver.rs:344-346, 421-426    */
  CFD_ERR_DIAGONAL = 4,   /* "Diagonal not found in CSR cols": init/mesh.rs:210   */
  CFD_ERR_RCCL = 5,       /* collective failure (distributed solver)            */
  CFD_ERR_INTERNAL = 6
} cfd_status;

const char* cfd_last_error(void);
/* Source hash of this build (sha256 prefix over csrc/ and include/, computed by
 * __graft_entry__.source_hash()); no reference counterpart -- it ties every
 * measured number to the code that produced it. */
const char* cfd_build_id(void);

/* ------------------------------------------------------------------------ */
/* Mesh (input format).  Mirrors `Mesh` SoA, src/solver/mesh/structs.rs:12-42.
 * face_neighbor == UINT32_MAX marks a boundary face (Option<usize>::None,
 * init/mesh.rs:63-70); face_boundary: 0 none, 1 inlet, 2 outlet, 3 wall
 * (init/mesh.rs:76-84).  Geometry is f64 and is rounded to f32 on upload
 * exactly like init/mesh.rs:93-155.                                          */
typedef struct cfd_mesh_view {
  uint32_t num_cells;
  uint32_t num_faces;
  const uint32_t* face_owner;        /* [num_faces]     */
  const uint32_t* face_neighbor;     /* [num_faces]     */
  const uint32_t* face_boundary;     /* [num_faces]     */
  const double* face_area;           /* [num_faces]     */
  const double* face_nx;             /* [num_faces]     */
  const double* face_ny;             /* [num_faces]     */
  const double* face_cx;             /* [num_faces]     */
  const double* face_cy;             /* [num_faces]     */
  const double* cell_cx;             /* [num_cells]     */
  const double* cell_cy;             /* [num_cells]     */
  const double* cell_vol;            /* [num_cells]     */
  const uint32_t* cell_face_offsets; /* [num_cells + 1] */
  const uint32_t* cell_faces;        /* [cell_face_offsets[num_cells]] */
} cfd_mesh_view;

/* Geometry of the reference mesher (src/solver/mesh/geometry.rs).           */
typedef struct cfd_geometry {
  int32_t kind;  /* 0 BackwardsStep{length,h_in,h_out,step_x}
                    1 ChannelWithObstacle{length,height,cx,cy,r}
                    2 RectangularChannel{length,height}
                    3 CircleObstacle{cx,cy,r,xmin,ymin,xmax,ymax} (mesh/tests.rs) */
  double p[8];
} cfd_geometry;

typedef struct cfd_mesh cfd_mesh; /* owned host mesh */

/* generate_cut_cell_mesh (src/solver/mesh/cut_cell.rs:10-16)               */
cfd_status cfd_mesh_generate_cut_cell(const cfd_geometry* geo, double min_cell_size,
                                      double max_cell_size, double growth_rate,
                                      double domain_x, double domain_y, cfd_mesh** out);
/* generate_voronoi_mesh (src/solver/mesh/voronoi.rs:23, delaunay.rs): a
 * behavioural restatement with a SEEDED generator (the reference's
 * thread_rng is unseeded): Poisson-disk generators graded like the cut-cell
 * sizing, Bowyer-Watson Delaunay, 20 generator-smoothing sweeps, polygonal
 * dual cells.  Same seed and arguments: the same mesh.  Geometry kinds 0-3. */
cfd_status cfd_mesh_generate_voronoi(const cfd_geometry* geo, double min_cell_size,
                                     double max_cell_size, double growth_rate, double domain_x,
                                     double domain_y, uint64_t seed, cfd_mesh** out);
/* generate_delaunay_mesh (delaunay.rs:732): the same seeded triangulation
 * with the triangles as cells.                                             */
cfd_status cfd_mesh_generate_delaunay(const cfd_geometry* geo, double min_cell_size,
                                      double max_cell_size, double growth_rate, double domain_x,
                                      double domain_y, uint64_t seed, cfd_mesh** out);
/* Mesh::smooth (structs.rs:159-292); returns iterations done in *iters.     */
cfd_status cfd_mesh_smooth(cfd_mesh* m, const cfd_geometry* geo, double target_skew,
                           int32_t max_iterations, int32_t* iters);
/* Mesh::calculate_max_skewness (structs.rs:294-320)                         */
double cfd_mesh_max_skewness(const cfd_mesh* m);
/* Borrowed view of the mesh arrays (valid until the mesh is modified/freed). */
cfd_status cfd_mesh_get_view(const cfd_mesh* m, cfd_mesh_view* out);
/* Vertex arrays (vx, vy, v_fixed) for mesh-validity tests.                  */
cfd_status cfd_mesh_get_vertices(const cfd_mesh* m, uint32_t* num_vertices, const double** vx,
                                 const double** vy, const uint8_t** v_fixed);
/* Vertex topology (structs.rs face_v1/face_v2, cell_vertex_offsets[N+1],
 * cell_vertices: CCW polygon of each cell) for mesh-validity tests.        */
cfd_status cfd_mesh_get_topology(const cfd_mesh* m, const uint32_t** face_v1, const uint32_t** face_v2,
                                 const uint32_t** cell_vertex_offsets, const uint32_t** cell_vertices);
/* Binary SoA dump / load.                              */
cfd_status cfd_mesh_save(const cfd_mesh* m, const char* path);
cfd_status cfd_mesh_load(const char* path, cfd_mesh** out);
void cfd_mesh_destroy(cfd_mesh* m);

/* ------------------------------------------------------------------------ */
/* Constants: same 14-field layout as GpuConstants (structs.rs:86-101).      */
typedef struct cfd_constants {
  float dt;
  float dt_old;
  float time;
  float viscosity;
  float density;
  uint32_t component;
  float alpha_p;
  uint32_t scheme;      /* 0 Upwind, 1 SOU, 2 QUICK (scheme.rs)  */
  float alpha_u;
  uint32_t stride_x;
  uint32_t time_scheme; /* 0 Euler, 1 BDF2                       */
  float inlet_velocity;
  float ramp_time;
  uint32_t precond_type; /* 0 Jacobi, 1 AMG (PreconditionerType) */
} cfd_constants;

/* Build-side configuration (hard-coded numerics of the reference). */
typedef struct cfd_config {
  int32_t n_outer_correctors; /* 20 (init/mod.rs:144)                                  */
  int32_t convergence_lag;    /* 1 = reference async-read model (default), 0 = exact  */
  int32_t fixed_outer;        /* >0: exactly this many Picard iterations, no early exit */
  int32_t fixed_inner;        /* >0: exactly this many FGMRES iterations per solve     */
  int32_t max_restart;        /* 50  (coupled_solver_fgmres.rs:1737)                   */
  int32_t max_outer_restarts; /* 20  (coupled_solver_fgmres.rs:1738)                   */
  float fgmres_rtol;          /* 1e-5                                                   */
  float fgmres_atol;          /* 1e-7                                                   */
  int32_t log_level;          /* 0 silent; 1 the reference's println! progress lines
                                 (coupled_solver.rs, coupled_solver_fgmres.rs) on stderr,
                                 rank 0 only; 2 also AMG setup timings; 3 also a stream
                                 synchronisation + error check after every kernel phase
                                 (debug: a fault is reported where it happened)          */
  int32_t amg_rebuild_interval; /* 0: AMG hierarchy frozen after the first AMG solve
                                   (reference, amg.rs); k > 0: rebuilt from the current
                                   matrix every k steps (opt-in deviation) */
  int32_t amg_local_aggregation; /* distributed solver only.  0 (default): the GLOBAL
                                   hierarchy -- the reference's greedy index-order
                                   aggregation over the whole mesh, aggregates may
                                   straddle ranks, R ranks give one GPU's bits.  1:
                                   partition-aware -- each row-partitioned level is
                                   aggregated over the rank's own rows only (cross-rank
                                   entries ignored by the greedy pass):
                                   block-diagonal P / R, so the restriction and the
                                   prolongation need no halo; the hierarchy (and the
                                   bits) then depend on the rank count, and match the
                                   oracle run with the same rank count and mode       */
  float comm_timeout_s;          /* distributed solver (RCCL and host-staged transports):
                                   progress watchdog.  An operation of the transport still
                                   incomplete after this many seconds, or an asynchronous
                                   RCCL error (ncclCommGetAsyncError), makes a background
                                   thread print the rank, device, operation and category
                                   on stderr, abort the communicator (ncclCommAbort) and
                                   end the process with status 70.  Default 180; <= 0 off.
                                   No reference counterpart (the reference is one GPU).  */
} cfd_config;

void cfd_config_default(cfd_config* cfg);

typedef struct cfd_linear_stats { /* LinearSolverStats, structs.rs:11-18 */
  uint32_t iterations;
  float residual;
  int32_t converged;
  int32_t diverged;
  double time_s;
} cfd_linear_stats;

typedef struct cfd_step_info {
  int32_t should_stop;
  uint32_t degenerate_count;
  uint32_t steady_state_count;
  float outer_residual_u;
  float outer_residual_p;
  uint32_t outer_iterations;
  cfd_linear_stats stats_p; /* the only stats field the reference writes */
  uint32_t total_linear_iterations; /* summed over the step's outer iterations */
} cfd_step_info;

typedef struct cfd_solver cfd_solver;

/* GpuSolver::new (init/mod.rs:15-19).  hip_device selects the GPU.           */
cfd_status cfd_solver_create(const cfd_mesh_view* mesh, const cfd_config* cfg, int32_t hip_device,
                             cfd_solver** out);
void cfd_solver_destroy(cfd_solver* s);

/* solver.rs:9-34: each call overwrites the WHOLE state (other fields = 0).   */
cfd_status cfd_set_u(cfd_solver* s, const double* uv /* [2N] interleaved */);
cfd_status cfd_set_p(cfd_solver* s, const double* p /* [N] */);
/* `constants` public field: host copy; takes effect at update_constants/step */
cfd_status cfd_get_constants(const cfd_solver* s, cfd_constants* out);
cfd_status cfd_set_constants(cfd_solver* s, const cfd_constants* c);
/* setters, solver.rs:36-95 (set_dt keeps the dt_old rule)                    */
cfd_status cfd_set_dt(cfd_solver* s, float dt);
cfd_status cfd_set_viscosity(cfd_solver* s, float nu);
cfd_status cfd_set_alpha_p(cfd_solver* s, float a);
cfd_status cfd_set_alpha_u(cfd_solver* s, float a);
cfd_status cfd_set_density(cfd_solver* s, float rho);
cfd_status cfd_set_scheme(cfd_solver* s, uint32_t scheme);
cfd_status cfd_set_time_scheme(cfd_solver* s, uint32_t scheme);
cfd_status cfd_set_inlet_velocity(cfd_solver* s, float v);
cfd_status cfd_set_ramp_time(cfd_solver* s, float t);
cfd_status cfd_set_precond_type(cfd_solver* s, uint32_t precond_type);
cfd_status cfd_update_constants(cfd_solver* s);
/* solver.rs:276-294                                                          */
cfd_status cfd_initialize_history(cfd_solver* s);
/* solver.rs:242 -> coupled_solver.rs:33-499                                  */
cfd_status cfd_step(cfd_solver* s);
/* Waits until the handle's GPU is idle (hipDeviceSynchronize on its device):
 * the timing fence bench.py puts on both sides of the timed steps.          */
cfd_status cfd_synchronize(cfd_solver* s);
/* solver.rs:97-128 (blocking)                                               */
cfd_status cfd_get_u(cfd_solver* s, double* uv /* [2N] */);
cfd_status cfd_get_p(cfd_solver* s, double* p /* [N] */);
cfd_status cfd_get_d_p(cfd_solver* s, double* dp /* [N] */);
cfd_status cfd_get_step_info(const cfd_solver* s, cfd_step_info* out);
/* The caller-writable part of the step info: the reference's public fields
 * should_stop / degenerate_count / steady_state_count (structs.rs:244-247),
 * which the GUI writes between steps (src/ui/app.rs:852-857: should_stop =
 * false before it resumes) and check_evolution then reads and updates
 * (coupled_solver.rs:553-578).  Distributed solver: call it on every rank
 * with the same values (the counters are global).                          */
cfd_status cfd_set_stop_state(cfd_solver* s, int32_t should_stop, uint32_t degenerate_count,
                              uint32_t steady_state_count);
/* The reference's public field n_outer_correctors (structs.rs:238, 20 from
 * init/mod.rs:144), read by every step_coupled (coupled_solver.rs:111: at
 * least 10 Picard iterations) -- caller-writable between steps like the stop
 * state; cfd_config.n_outer_correctors is its initial value.  n >= 0.       */
cfd_status cfd_set_n_outer_correctors(cfd_solver* s, int32_t n);
uint32_t cfd_num_cells(const cfd_solver* s);
uint32_t cfd_num_faces(const cfd_solver* s);

/* ------------------------------------------------------------------------ */
/* Checkpoint / resume (the reference keeps its state only in GPU
 * buffers, get_u/get_p being its only export).  The file holds everything a
 * step reads from earlier steps, in f32 exactly as the device holds it, so a
 * solver that loads it steps bit-identically to the one that saved it:
 *   header (cfd_state_file_header, 512 bytes), then GLOBAL per-cell arrays
 *   (cell order of the mesh, independent of the rank count):
 *   ring slot 0, 1, 2: u f32[2N] (interleaved), p f32[N], d_p f32[N],
 *                      grad_p f32[2N]                (FluidState x3, structs.rs)
 *   prev (check_evolution snapshot): the same four arrays
 *   x f32[3N]  (FGMRES solution = initial guess of the next solve)
 *   if amg_nnz > 0: amg_rowptr u64[N+1], amg_val f32[amg_nnz] -- the scalar
 *   pressure matrix the AMG hierarchy was built from (CSR, columns ascending;
 *   the pattern is the mesh's), so the loader rebuilds the same hierarchy --
 *   under the LOADER's aggregation mode and rank count: the default (global)
 *   hierarchy is rank-count independent; a partition-aware one
 *   (amg_local_aggregation = 1) depends on the rank count, so a file saved
 *   in that mode continues bit-identically only on the same rank count and
 *   mode.  The loader prints a warning on stderr when they differ.          */
typedef struct cfd_state_file_header {
  char magic[8];        /* "CFD2STAT" */
  uint32_t version;     /* 1 */
  uint32_t header_bytes; /* 512 */
  uint64_t num_cells;
  uint64_t num_faces;
  uint64_t amg_nnz;     /* 0: no AMG hierarchy built when saved */
  int32_t step_index;   /* ring rotation (coupled_solver.rs:43-71) */
  int32_t have_prev;
  int32_t inner_has_last; /* FGMRES lagged residual read (async_buffer.rs) */
  float inner_last;
  uint32_t n_variance;  /* entries of variance[] in use (<= 10), oldest first */
  uint32_t reserved0;
  double variance[10][2]; /* check_evolution's (var_u, var_v) history */
  cfd_constants constants;
  cfd_step_info info;
  uint32_t amg_age;     /* steps since the hierarchy was built (amg_rebuild_interval) */
  int32_t amg_local_aggregation; /* cfd_config.amg_local_aggregation of the saving run */
  int32_t nranks;       /* rank count of the saving run (0: not recorded)             */
  uint8_t reserved[164];
} cfd_state_file_header;

/* Writes the state to `path`.  Distributed solver: COLLECTIVE, every rank
 * writes its owned cells into the same file (one node: one filesystem).    */
cfd_status cfd_state_save(cfd_solver* s, const char* path);
/* Replaces the state with the file's (not collective: a distributed rank
 * reads its owned cells and ghosts).  The file may come from any rank
 * count.  The solver's own AMG hierarchy, if built, is dropped; the saved
 * scalar matrix, if any, is what the next AMG solve rebuilds it from.      */
cfd_status cfd_state_load(cfd_solver* s, const char* path);
/* In-process group: cfd_state_save on every rank (one host thread each).   */
cfd_status cfd_group_state_save(cfd_solver* const* handles, int32_t nranks, const char* path);

/* ------------------------------------------------------------------------ */
/* Instrumentation (replaces profiling.rs): HIP-event timing of the level-0
 * AMG smoother sweep, on the solver's own stream.                            */
cfd_status cfd_profile_enable(cfd_solver* s, int32_t enable);
cfd_status cfd_profile_reset(cfd_solver* s);
/* total_ms / launches over the level-0 smoother sweeps since
 * cfd_profile_reset (every sweep timed while profiling is on); bytes =
 * algorithmic bytes per sweep (4(n+1) + 8 nnz + 12 n).       */
cfd_status cfd_profile_smoother(const cfd_solver* s, double* total_ms, uint64_t* launches,
                                double* bytes_per_launch);
/* hipGraph replay of the FGMRES iteration (one executable graph per basis
 * index, captured on first use, replayed by every later solve; DESIGN.md
 * section 5).  enable: 1 on, 0 off (the launches are issued one by one);
 * default off: replay measured no faster than
 * eager launches.  One GPU only.  Same bits either
 * way.  Stats: graphs captured and iterations replayed so far.             */
cfd_status cfd_graph_enable(cfd_solver* s, int32_t enable);
cfd_status cfd_graph_stats(const cfd_solver* s, int32_t* enabled, uint64_t* captures, uint64_t* replays);
/* AMG hierarchy summary: number of levels and rows/nnz per level.            */
cfd_status cfd_amg_levels(const cfd_solver* s, int32_t* num_levels, uint32_t* rows /*[20]*/,
                          uint64_t* nnz /*[20]*/);
/* AMG setup path taken (0 not built yet, 1 host, 2 device; SURVEY §8(f)
 * rank 3) and an FNV-1a digest of every byte of level `level`'s device image
 * (matrix, diagonal, P, R) -- host and device setups must agree bit-for-bit.
 * Debug/parity only; not part of the reference surface.                     */
cfd_status cfd_debug_amg_info(cfd_solver* s, int32_t level, int32_t* setup_path, uint64_t* digest);
/* Which column form the row kernels of this handle read: 1 = 16-bit deltas
 * (col - row), 0 = 32-bit absolute columns.  coupled_use16: the coupled
 * matrix and every kernel over the mesh topology; level_use16[i]: AMG level i
 * (num_levels of them, 0 before the hierarchy is built).  Reads host fields
 * only: allocates nothing, launches nothing.  Debug/parity only.            */
cfd_status cfd_debug_column_widths(const cfd_solver* s, int32_t* coupled_use16, int32_t* num_levels,
                                   int32_t* level_use16 /*[20]*/);
/* One level of the built AMG hierarchy as plain CSR, expanded from the device
 * image the V-cycle kernels read (ELL values, 16/32-bit columns, u8 / u16 row
 * lengths and diagonal ranks, dv, de, agg, R, r_m4), never from a host copy
 * kept by the setup.  Two calls: with every pointer NULL the call fills the
 * sizes (n, nnz, nc, r_nnz, wide, use16); with the arrays allocated to those
 * sizes it fills them (a NULL array is skipped).  row/col/val: columns
 * ascending, the diagonal included (value dv); agg, r_row, r_col, m4, m4_more
 * only when nc > 0 (the level has a coarse level).  m4[4 I + q]: member q of
 * aggregate I as the r_m4 image lists it (-1: none); m4_more[I]: 1 when the
 * image flags more than four members.  Debug/parity only; one GPU only (a
 * distributed handle, no hierarchy, or no such level: CFD_ERR_INVALID).     */
typedef struct cfd_amg_level {
  uint32_t n;       /* rows                                                  */
  uint32_t nc;      /* aggregates (rows of the next level); 0: last level    */
  uint64_t nnz;     /* entries of row/col/val, diagonal included             */
  uint64_t r_nnz;   /* entries of r_col (= n when every row has an aggregate) */
  int32_t wide;     /* 1: 16-bit row lengths (tail kernels only)             */
  int32_t use16;    /* 1: 16-bit column deltas                               */
  uint32_t* row;    /* [n + 1]                                               */
  uint32_t* col;    /* [nnz]                                                 */
  float* val;       /* [nnz]                                                 */
  float* dv;        /* [n] raw diagonal                                      */
  float* de;        /* [n] smoother diagonal                                 */
  uint32_t* agg;    /* [n]                                                   */
  uint32_t* r_row;  /* [nc + 1]                                              */
  uint32_t* r_col;  /* [r_nnz]                                               */
  int32_t* m4;      /* [4 nc]                                                */
  int32_t* m4_more; /* [nc]                                                  */
} cfd_amg_level;
cfd_status cfd_debug_amg_level(cfd_solver* s, int32_t level, cfd_amg_level* io);
/* One application of the AMG V-cycle outside the solve: uploads x0 to the
 * level-0 solution vector and b to its right-hand side, runs exactly the cycle
 * the preconditioner runs (the planned schedule under the knobs in force; the
 * plain cycle when reference semantics 1 / 8 are on), synchronises and returns
 * the solution vector.  Never inside a captured graph; touches only those two
 * vectors and the level scratch, so a later step gives the bits of a solver
 * that never called it.  n must be cfd_num_cells.  Needs a built hierarchy;
 * debug/parity only; one GPU only (else CFD_ERR_INVALID).                    */
cfd_status cfd_debug_amg_vcycle(cfd_solver* s, const float* x0, const float* b, float* x_out, size_t n);
/* One application of the FGMRES preconditioner outside the solve: z = M^-1 v
 * for v, z of 3 cfd_num_cells floats (u, v, p per cell), exactly as an
 * iteration applies it (Schur prediction, V-cycle or Jacobi relaxation by
 * precond_type, velocity correction) on the matrices of the last assembly.
 * Uses the first Krylov basis / Z slots and the pressure scratch, all of which
 * the next solve rewrites before reading: a later step keeps its bits.  Needs
 * a completed step (and, with precond_type 1, a built hierarchy); debug/parity
 * only; one GPU only (else CFD_ERR_INVALID).                                 */
cfd_status cfd_debug_apply_precond(cfd_solver* s, const float* v, float* z, size_t n3);
/* Layout-true bytes of one level-0 smoother sweep: the minimum the kernel
 * moves in this library's level image (u8 lengths, ELL values + 16/32-bit
 * columns, b, x, diagonal, x_out); the roofline of record divides this by
 * the measured sweep time (cfd_profile_smoother's bytes are the reference
 * CSR format's count).                                        */
double cfd_smoother_layout_bytes(const cfd_solver* s);
/* Layout-true bytes of one step under the fixed schedule: every kernel's
 * minimum traffic in this library's layouts (a lower bound of the HBM bytes,
 * unlike the reference-format count below) times its launches per step.    */
double cfd_step_layout_bytes(const cfd_solver* s);
/* Algorithmic bytes of one step under the fixed schedule in the reference's
 * CSR/f32/u32 format -- a count, larger than this layout's
 * traffic.                                                                  */
double cfd_step_algorithmic_bytes(const cfd_solver* s);

/* Debug/parity access to internal device buffers, copied to host.
 * ids: 0 fluxes-by-face[F], 1 grad_u[2N], 2 grad_v[2N], 3 rhs[3N], 4 x[3N],
 * 5 diag_u_inv[N], 6 diag_v_inv[N], 7 diag_p_inv[N], 8 scalar_matrix[nnz_s],
 * 9 coupled_matrix_csr[9 nnz_s] (reference CSR order), 10 grad_p[2N],
 * 11 state_old u[2N], 12 state_old_old u[2N]                                 */
cfd_status cfd_debug_buffer(cfd_solver* s, int32_t id, float* out, size_t count);
size_t cfd_debug_buffer_len(const cfd_solver* s, int32_t id);
/* Runs only prepare_coupled (+ coupled_assembly_merged when assemble != 0) on
 * the current state without rotating the ring (kernel-level parity).        */
cfd_status cfd_debug_prepare_assemble(cfd_solver* s, int32_t assemble);
/* Test mode: the reference's own semantics under a legal schedule instead of
 * the canonical resolutions, with the oracle's flag bits
 * (oracle_set_semantics): 4 the reference's reduction order -- 64-DOF
 * workgroup trees, then reduce_final's serial sum (norms, gmres_ops.wgsl:
 * 241-293) or reduce_dots_cgs's strided lanes + tree (CGS, gmres_cgs.wgsl:
 * 86-120), and check_evolution's serial f64 loops (coupled_solver.rs:504-545)
 * on the host; 1 the in-place AMG smoother (amg.wgsl:24-50) with its 64-row
 * workgroups run in order; 2 prepare_coupled's racy neighbour reads
 * (prepare_coupled.wgsl:140-143 vs :328-337), its 64-cell workgroups in order,
 * the assembly reading each face's flux as its owner stored it; 8
 * restrict_residual's out-of-bounds rows (amg.rs:707-719) under wgpu's
 * Restrict policy.  Flags 4 give the bits of the reference's WGSL kernels run
 * with the whole dispatch resident, 13 those with the V-cycle's workgroups in
 * order, 15 those with every dispatch's workgroups in order
 * (tests/test_gpu_wgsl_pin.py).  Other bits, or a distributed handle:
 * CFD_ERR_INVALID.  Slow (serial sums / workgroups); drops captured graphs;
 * 0 = canonical.                                                            */
cfd_status cfd_debug_reference_semantics(cfd_solver* s, int32_t flags);

/* ------------------------------------------------------------------------ */
/* Multi-GPU (the reference is single-GPU).  The mesh is split
 * into R contiguous cell ranges (x-major cut-cell numbering => vertical
 * slabs), rank r owning [floor(N r/R), floor(N (r+1)/R)).  Ghost-cell halos
 * of the state, the Krylov vectors and every distributed AMG level go to the
 * slab neighbours; reductions all-gather per-rank partial sums and add them
 * in rank order (deterministic, identical on every rank).  For a distributed
 * handle: `mesh` is the WHOLE mesh on every rank; cfd_set_u/cfd_set_p take
 * the global arrays; cfd_num_cells and cfd_get_u/p/d_p cover the owned cells.
 *
 * One process per GPU over RCCL (the production path): rank 0 calls
 * cfd_dist_unique_id and broadcasts the 128 bytes (e.g. torch.distributed);
 * every rank then calls cfd_solver_create_dist (collective) and steps with
 * cfd_step (collective).                                                    */
cfd_status cfd_dist_unique_id(uint8_t out[128]);
cfd_status cfd_solver_create_dist(const cfd_mesh_view* mesh, const cfd_config* cfg,
                                  int32_t hip_device, int32_t nranks, int32_t rank,
                                  const uint8_t unique_id[128], cfd_solver** out);
/* Host-staged transport (test / rehearsal mode, e.g. several processes on
 * ONE GPU, where RCCL refuses a second rank per device): the same
 * distributed solver, with every halo exchange and all-gather staged through
 * host memory and handed to caller callbacks (bench.py binds them to
 * torch.distributed's gloo backend).  exchange: transfers with the same peer
 * match in list order, send k of one rank with receive k of the other;
 * allgather: recv[r * bytes ...] = rank r's send.  Callbacks return 0 on
 * success.  Not a performance path.                                          */
typedef int32_t (*cfd_exchange_fn)(void* user, int32_t n, const int32_t* peer, void* const* send,
                                   const uint64_t* send_bytes, void* const* recv, const uint64_t* recv_bytes);
typedef int32_t (*cfd_allgather_fn)(void* user, void* send, void* recv, uint64_t bytes);
cfd_status cfd_solver_create_dist_host(const cfd_mesh_view* mesh, const cfd_config* cfg, int32_t hip_device,
                                       int32_t nranks, int32_t rank, cfd_exchange_fn exchange,
                                       cfd_allgather_fn allgather, void* user, cfd_solver** out);
/* In-process group (SURVEY §8(b) `cfd_solver_create_dist(..., nranks,
 * devices)`): nranks handles in this process, rank r on devices[r] (devices
 * may repeat: all ranks on one GPU is allowed).  Collective calls go through
 * cfd_group_step / cfd_group_debug_prepare_assemble (one host thread per rank). */
cfd_status cfd_group_create(const cfd_mesh_view* mesh, const cfd_config* cfg, int32_t nranks,
                            const int32_t* devices, cfd_solver** out /* [nranks] */);
cfd_status cfd_group_step(cfd_solver* const* handles, int32_t nranks);
/* A cfd_group_step that failed on any rank leaves the ranks at different
 * points of the step, so the group is marked "needs restore": further
 * cfd_group_step calls return CFD_ERR_INVALID until every rank has loaded a
 * consistent state (cfd_state_load, per rank) or the caller accepts the state
 * as is (cfd_group_reset).  cfd_group_needs_restore: 1 while marked.       */
cfd_status cfd_group_reset(cfd_solver* const* handles, int32_t nranks);
int32_t cfd_group_needs_restore(cfd_solver* const* handles, int32_t nranks);
/* RCCL plumbing check on one GPU: 1-rank communicator, grouped send/recv to
 * self and an all-gather through the solver's transport; CFD_OK if the data
 * arrived intact.                                                           */
cfd_status cfd_debug_rccl_selftest(int32_t hip_device);
/* Progress-watchdog self-test, no GPU needed: a watchdog with limit
 * `timeout_s` around a host-blocking operation that takes `hang_ms`.  If
 * hang_ms exceeds the limit, the watchdog ends the PROCESS with status 70
 * (as on a stalled collective; run it in a child process); else CFD_OK.    */
cfd_status cfd_debug_comm_watchdog(float timeout_s, int32_t hang_ms);
/* Transport of a distributed handle and its traffic since the last reset
 * (bench.py prints these on a --gpus N line).                               */
typedef struct {
  int32_t transport;        /* 0 none (one rank), 1 RCCL, 2 in-process group, 3 host-staged */
  int32_t comm_count;       /* RCCL: ncclCommCount; otherwise the rank count */
  int32_t comm_rank;        /* RCCL: ncclCommUserRank; otherwise the rank */
  int32_t device;           /* HIP device of this rank */
  uint64_t exchanges;       /* grouped point-to-point calls (halos) */
  uint64_t allgathers;      /* all-gather calls (reductions, replicated AMG levels) */
  uint64_t bytes_sent;      /* point-to-point payload bytes this rank sent */
  uint64_t bytes_gathered;  /* all-gather payload bytes this rank contributed */
} cfd_comm_stats;
cfd_status cfd_dist_comm_stats(cfd_solver* s, cfd_comm_stats* out, int32_t reset);
/* Timing of the distributed communication by category (measurement aid for
 * the multi-GPU runs; no reference counterpart).  While enabled, every halo
 * exchange and all-gather is bracketed by timing events (a small cost:
 * bench.py times its headline steps with it off, then one extra step with it
 * on).  category: 0 Krylov halos (V_j, p_sol, Z_j, x), 1 state / assembly
 * halos, 2 reduction all-gathers (dots, norms, max-diff), 3 the all-gather of
 * the first replicated AMG level's rhs, 4 AMG level halos (`level` = the AMG
 * level).  wait_us: time the compute stream stood still for the operation
 * (halos: from reaching the wait on the exchange to its release; all-gathers
 * run on the compute stream: their whole duration); comm_us: the
 * transport's own time (halos: the grouped send/recv on the comm stream,
 * peer waits included).  enable resets the totals.                         */
typedef struct {
  int32_t category;
  int32_t level;    /* AMG level (category 4), else -1 */
  uint64_t calls;
  uint64_t bytes;   /* payload this rank sent / contributed */
  double wait_us;
  double comm_us;
} cfd_comm_timing_entry;
cfd_status cfd_comm_timing_enable(cfd_solver* s, int32_t enable);
/* the non-empty categories, at most `cap`; *count = how many were written  */
cfd_status cfd_comm_timing(cfd_solver* s, cfd_comm_timing_entry* out, int32_t cap, int32_t* count);
/* In-process group failure path (test hook): every rank enters a collective
 * except `fail_rank`, which fails first; the others must return an error
 * instead of waiting forever, and the group must stay usable afterwards.     */
cfd_status cfd_debug_group_fault(cfd_solver* const* handles, int32_t nranks, int32_t fail_rank);
/* ... and a failure in the middle of a step: `fail_rank` throws right after
 * the step's first prepare() while the other ranks continue until their next
 * collective; the group is then marked needs-restore (see cfd_group_reset). */
cfd_status cfd_debug_group_fault_midstep(cfd_solver* const* handles, int32_t nranks, int32_t fail_rank);
/* rank, rank count, owned global range [c0, c1), global cell count         */
cfd_status cfd_dist_info(const cfd_solver* s, int32_t* rank, int32_t* nranks, uint32_t* c0,
                         uint32_t* c1, uint32_t* num_global_cells);
/* Host-only halo plan of rank `rank` (no GPU needed; for tests / tooling).
 * First call with null arrays to get the sizes.  ghost_global: ghost cell ids
 * (ascending); per peer: peer rank, recv count, send count; send_global: the
 * owned cell ids sent to each peer, concatenated in peer order.            */
cfd_status cfd_dist_plan(const cfd_mesh_view* mesh, int32_t nranks, int32_t rank, uint32_t* c0,
                         uint32_t* c1, uint32_t* num_ghosts, uint32_t* num_peers,
                         uint32_t* num_send, uint32_t* ghost_global, int32_t* peer_rank,
                         uint32_t* peer_recv, uint32_t* peer_send, uint32_t* send_global);

/* ------------------------------------------------------------------------ */
/* Flow diagnostics, derived fields and the adaptive time step: what the
 * reference's driver loop does on the host after every step (src/ui/app.rs:
 * 871-910: read u back, max_vel = max sqrt(vx^2 + vy^2), dt = target_cfl *
 * min_cell_size / max_vel limited to 1.2x growth and [1e-9, 100]) as one
 * read-only pass over the current state on the GPU.  Nothing cfd_step reads is
 * written; a handle that never calls these launches and allocates nothing.
 * Per cell, in f32 with the step's own arithmetic: the Green-Gauss velocity
 * gradients g_u, g_v exactly as prepare_coupled forms them (inlet face value
 * inlet_velocity * smoothstep(0, ramp_time, time) of the current constants,
 * wall 0, outlet the cell value), omega = g_v.x - g_u.y, div = g_u.x + g_v.y.
 * Maxima ignore NaN cells (the reference's `if v > max_vel`).  Sums are f64
 * in the canonical reduction order, so a distributed solver returns one
 * GPU's bits on every rank.
 * Wall force: of the fluid on the wall faces selected by cfd_set_force_region,
 * consistent with the assembly (wall face pressure = cell pressure, wall
 * diffusion = viscosity * area / |face centre - cell centre|), n out of the
 * cell: pressure sum p n area, viscous sum viscosity * u * area / dist.  With
 * buoyancy on (the last section) p carries the hydrostatic part, so the
 * pressure force contains the buoyant lift of the selected walls.           */
typedef struct cfd_flow_diag {
  double max_speed;        /* sqrt (host, f64) of the device max of (double)u u + (double)v v: the reference's max_vel */
  double max_vorticity;    /* max |omega_i| */
  double max_divergence;   /* max |div_i|   */
  double kinetic_energy;   /* sum 0.5 vol (u^2 + v^2)   (per unit density) */
  double enstrophy;        /* sum 0.5 vol omega^2 */
  double force_pressure[2];
  double force_viscous[2];
  uint32_t region_faces;   /* wall faces selected, whole mesh */
  uint32_t reserved;
} cfd_flow_diag;
/* Collective on a distributed handle (every rank gets the same bytes).      */
cfd_status cfd_flow_diagnostics(cfd_solver* s, cfd_flow_diag* out);
/* kind 0 speed, 1 vorticity, 2 divergence of the owned cells, widened to f64
 * (runs the pass with its field outputs on; not collective)                 */
cfd_status cfd_get_derived(cfd_solver* s, int32_t kind, double* out /* [N owned] */);
/* Selects the wall faces (boundary 3) whose f64 centre lies in the closed box
 * [x0, x1] x [y0, y1]; x1 < x0 selects none.  *faces (optional) = faces
 * selected over the whole mesh.  Distributed solver: call it on every rank
 * with the same box (not collective).                                       */
cfd_status cfd_set_force_region(cfd_solver* s, double x0, double y0, double x1, double y1, uint32_t* faces);
/* min sqrt(cell_vol), f64, over the WHOLE mesh (app.rs:377-381); 0 for null */
double cfd_min_cell_size(const cfd_solver* s);
/* app.rs:897-909 in f64, no handle: *changed = 0 and *next_dt = current_dt
 * unless max_vel > 1e-6; else next = target_cfl * min_cell_size / max_vel,
 * capped at current_dt * 1.2, clamped to [1e-9, 100].                       */
cfd_status cfd_adaptive_dt_rule(double current_dt, double target_cfl, double min_cell_size, double max_vel,
                                double* next_dt, int32_t* changed);
/* cfd_flow_diagnostics -> the rule with current_dt = (double)constants.dt ->
 * cfd_set_dt((float)next) (which keeps the dt_old rule); *new_dt (optional) =
 * constants.dt afterwards.  Collective on a distributed handle: every rank
 * sets the same value.                                                      */
cfd_status cfd_adapt_dt(cfd_solver* s, double target_cfl, float* new_dt);
/* In-process group: the two collectives on every rank (one host thread
 * each).  They do not change the state, so a failure never marks the group
 * needs-restore; a group already marked returns CFD_ERR_INVALID.            */
cfd_status cfd_group_flow_diagnostics(cfd_solver* const* handles, int32_t nranks, cfd_flow_diag* out /* [nranks] */);
cfd_status cfd_group_adapt_dt(cfd_solver* const* handles, int32_t nranks, double target_cfl, float* new_dt);

/* ------------------------------------------------------------------------ */
/* Passive scalar transport: up to 4 fields phi_f (dye, temperature,
 * concentration) on the solver's mesh, advected by the conservative mass
 * fluxes the last cfd_step left on the device and diffused with D_f.  Opt-in:
 * a handle that never calls cfd_scalars_enable allocates and launches nothing
 * new, and cfd_step launches none of it in any case.  Nothing cfd_step reads
 * is written; cfd_step only records, on the host, the dt it used.
 * The flux is that of the last k_prepare launch: the last Picard iteration's
 * of the last cfd_step, formed from the state before that iteration's update
 * (cfd_debug_prepare_assemble also refreshes it, from the current state).
 * Discretisation (all f32, every sum left to right in face-slot order; F_k the
 * mass flux out of cell i through its slot k, A_k the face area, d_k the
 * centre distance the momentum diffusion uses):
 *   time      a_t = vol_i * density / dt -- implicit Euler whatever
 *             constants.time_scheme says
 *   slot      c_k = max(-F_k, 0) + (density * D_f) * A_k / d_k on internal and
 *             inlet faces; 0 on walls (zero flux) and outlets (zero gradient;
 *             their flux is >= 0 by construction)
 *   system    (a_t + sum_k c_k) phi_i - sum_{internal k} c_k phi_other(k)
 *             = a_t phi_old_i + sum_{inlet k} c_k inlet_value
 *   solve     Jacobi from phi_old, in batches of check_interval sweeps, until
 *             max_i |phi^{m+1}_i - phi^m_i| <= tol or max_sweeps; running out
 *             of sweeps is not an error (converged = 0)
 * This is the bounded upwind form (div(u phi) - phi div(u)): every iterate is
 * a convex combination of phi_old_i, the neighbours and inlet_value, so a dye
 * in [0, 1] stays there up to rounding; the price is a conservation defect of
 * sum_i phi_i div_i dt (cfd_flow_diag.max_divergence bounds div_i).
 * One GPU only: handles of cfd_solver_create_dist* and members of a group
 * of more than one rank return CFD_ERR_INVALID from cfd_scalars_enable.
 * Checkpoints: cfd_state_save / cfd_state_load neither store nor touch the
 * scalar fields (the file format and its version are unchanged);
 * cfd_get_scalar / cfd_set_scalar round-trip the f32 values exactly, so a
 * caller can keep them next to the state file.                              */
typedef struct cfd_scalar_params {
  float diffusivity;   /* D_f >= 0 (kinematic; multiplied by density) */
  float inlet_value;   /* phi at inlet faces */
} cfd_scalar_params;
typedef struct cfd_scalar_config {
  float tol;               /* stop when max |phi^{m+1} - phi^m| <= tol; default 1e-6 */
  int32_t max_sweeps;      /* default 200; rounded up to a multiple of check_interval */
  int32_t check_interval;  /* default 4; >= 1 */
  int32_t reserved;
} cfd_scalar_config;
typedef struct cfd_scalar_stats {
  uint32_t sweeps;       /* of the last cfd_scalar_advance, this field */
  int32_t converged;
  float last_delta;
  float dt_used;
  double min, max;       /* f32 values widened (NaN cells ignored) */
  double integral;       /* sum vol * phi, f64, canonical order */
} cfd_scalar_stats;
void cfd_scalar_config_default(cfd_scalar_config* cfg);
/* (Re)allocates `count` fields, all zero, with params {0, 0}; count 0 frees
 * everything (later scalar calls then return CFD_ERR_INVALID).             */
cfd_status cfd_scalars_enable(cfd_solver* s, int32_t count /* 1..4; 0 frees */, const cfd_scalar_config* cfg /* null: defaults */);
cfd_status cfd_set_scalar_params(cfd_solver* s, int32_t field, const cfd_scalar_params* p);
cfd_status cfd_set_scalar(cfd_solver* s, int32_t field, const double* phi /* [N] */);
cfd_status cfd_get_scalar(cfd_solver* s, int32_t field, double* phi /* [N] */);
/* dt > 0: that step; dt <= 0: the dt the last cfd_step used (CFD_ERR_INVALID if none yet).
 * Advances every enabled field.  A NaN or infinite update returns
 * CFD_ERR_DIVERGED.                                                         */
cfd_status cfd_scalar_advance(cfd_solver* s, float dt);
cfd_status cfd_scalar_stats_get(cfd_solver* s, int32_t field, cfd_scalar_stats* out);

/* Solver of one scalar field.  Method 0 (the default) is the Jacobi loop
 * above, unchanged.  Method 1 runs BiCGStab on the Jacobi-scaled system first
 * and then the same Jacobi loop from its answer ("polish"), which alone
 * decides `converged`: it is for fields whose diffusion dominates on a fine
 * mesh (D dt / h^2 >> 1), where Jacobi needs thousands of sweeps.  A handle
 * that never selects method 1 allocates and launches nothing new; the first
 * selection allocates six work vectors, freed by cfd_scalars_enable(0).
 *
 * Arithmetic of method 1.  coef (c_k), diag and b are the assembled system
 * above; J(x)_i = (b_i + sum_k c_k x[o_k]) / diag_i is one Jacobi sweep (the
 * internal slots k in slot order, o_k the slot's neighbour, the sum starting
 * from b_i, a true division).  Vectors are f32 and every vector operation is
 * one f32 rounding per multiply, add, subtract or divide (nothing fused).
 *   operator  (A v)_i = v_i - (sum_k c_k v[o_k]) / diag_i, the sum over the
 *             internal slots in slot order starting from +0.0f
 *   dots      <a, b> = the canonical sum (the tree of cfd_scalar_stats.
 *             integral) of the f64 cell terms (double)a_i * (double)b_i
 *   scalars   rho, alpha, omega, beta are f64 on the device; a vector
 *             operation uses the f64 value rounded once to f32
 *   start     x = phi_old; r = J(x) - x; rh = r; p = r; rho = <rh, r>;
 *             res = max_i |r_i|.  res <= tol: stop, reason 1, iteration 0.
 *   iteration k = 1, 2, ...:
 *     a  v = A p;  d = <rh, v>;  alpha = rho / d.  If rho, d or f32(alpha) is
 *        zero or not finite: stop, reason 2, iteration k, x untouched.
 *     b  s = r - alpha v;  t = A s;  ts = <t, s>;  tt = <t, t>.
 *        tt == 0: x = x + alpha p; r = s; res = max |r|; stop, reason 2,
 *        iteration k.  Otherwise omega = ts / tt; if tt or f32(omega) is zero
 *        or not finite: stop, reason 2, iteration k, x untouched.
 *     c  x = (x + alpha p) + omega s;  r = s - omega t;  res = max_i |r_i|;
 *        rho' = <rh, r>.  res <= tol: stop, reason 1, iteration k.
 *        k == max_iters: stop, reason 3, iteration k.
 *     d  (the first coefficient of iteration k + 1)
 *        beta = (rho' / rho) * (alpha / omega), alpha and omega the f64
 *        values.  If rho' or f32(beta) is zero or not finite: stop, reason 2,
 *        iteration k + 1, x as step c left it.  Otherwise
 *        p = r + beta (p - omega v);  rho = rho'.
 *   max |r_i| is taken over f32 bit patterns, a NaN counting as +inf.
 * After a stop nothing is written any more: x is frozen bit for bit.  The
 * host launches iterations in batches of cfd_scalar_solver.check_interval and
 * reads the status words after each batch; x, the iteration count and the
 * reason do not depend on that interval.
 *   polish    from the frozen x, the Jacobi loop of method 0 with the handle's
 *             cfd_scalar_config: at least one batch of check_interval sweeps
 *             runs, and cfd_scalar_stats.sweeps / converged / last_delta
 *             describe it exactly as they describe method 0.  A non-finite
 *             update is CFD_ERR_DIVERGED, running out of sweeps converged = 0.
 * The iterates of the Krylov phase are not convex combinations; the final x
 * of a converged advance satisfies x_i <= J(x)_i + tol, so a dye in [0, 1]
 * stays within tol * max_i(diag_i / a_t,i) plus rounding of that interval.  */
typedef struct cfd_scalar_solver {
  int32_t method;          /* 0 Jacobi, 1 BiCGStab then Jacobi polish */
  int32_t max_iters;       /* BiCGStab iteration cap; default 500; >= 1 */
  int32_t check_interval;  /* iterations per host read; default 8; >= 1 */
  int32_t reserved;
} cfd_scalar_solver;
typedef struct cfd_scalar_solver_stats {
  int32_t method;          /* of the last cfd_scalar_advance, this field */
  int32_t iterations;      /* the iteration the Krylov phase stopped in; 0 for method 0 */
  int32_t stop_reason;     /* 1 residual, 2 breakdown, 3 max_iters; 0 for method 0 */
  uint32_t polish_sweeps;  /* == cfd_scalar_stats.sweeps for method 1; 0 for method 0 */
  float krylov_residual;   /* the last res of the Krylov phase (recursive residual) */
  int32_t reserved;
} cfd_scalar_solver_stats;
void cfd_scalar_solver_default(cfd_scalar_solver* cfg); /* method 0, 500, 8 */
/* Takes effect at the next cfd_scalar_advance.  CFD_ERR_INVALID: scalars not
 * enabled, a bad field index, a method other than 0 or 1, max_iters < 1,
 * check_interval < 1.  cfd_scalars_enable resets every field to method 0.   */
cfd_status cfd_set_scalar_solver(cfd_solver* s, int32_t field, const cfd_scalar_solver* cfg);
cfd_status cfd_scalar_solver_stats_get(cfd_solver* s, int32_t field, cfd_scalar_solver_stats* out);

/* Advection scheme of one scalar field.  Scheme 0 (the default) is the bounded
 * first-order upwind system above, unchanged.  Scheme 1, "limited linear", adds
 * a van Leer-limited linear-upwind face value as a deferred correction,
 * evaluated once per advance on phi_old and clamped so that the maximum
 * principle of scheme 0 still holds: coef (c_k) and diag are exactly scheme
 * 0's, only b changes, and the Jacobi loop, method 1 and the statistics run
 * unchanged on it.  A handle that never selects scheme 1 allocates and
 * launches nothing new, and cfd_step launches none of it in any case; the
 * first selection allocates one gradient (two f32 per cell) and a counter word
 * per field, freed by cfd_scalars_enable(0).
 *
 * Arithmetic of scheme 1.  All f32, one rounding per operation (nothing
 * fused), every sum left to right in face-slot order.  phi = phi_old; phi_i the
 * cell's own value, phi_o = phi[o_k] the neighbour's of internal slot k; F_k
 * the mass flux out of cell i through slot k; n_k = (nx, ny)_k the unit normal
 * out of cell i; A_k the area; lam_k the cell-side interpolation weight the
 * step's own gradients use, and "degenerate" its fallback flag (the two
 * centre-to-face distances add up to <= 1e-6); dv_k = (dvx, dvy)_k = the
 * neighbour's centre minus the cell's.
 *   gradient   face value vf_k:
 *                internal            lam_k * phi_i + (1 - lam_k) * phi_o
 *                internal, degenerate  0.5 * (phi_i + phi_o)
 *                inlet               inlet_value
 *                wall, outlet        phi_i
 *              gx = sum_k (vf_k * nx_k) * A_k, gy = sum_k (vf_k * ny_k) * A_k
 *              over every used slot, each from +0;  g_i = (gx / vol_i, gy /
 *              vol_i), true divisions.  Every g is formed before any is used.
 *   increment  per internal slot, h_k:
 *                F_k > 0 (cell i is upwind)    d = phi_o - phi_i
 *                                              gd = g_i.x * dvx_k + g_i.y * dvy_k
 *                F_k < 0 (the neighbour is)    d = phi_i - phi_o
 *                                              gd = -(g_o.x * dvx_k + g_o.y * dvy_k)
 *                otherwise (F_k == 0)          the slot is skipped
 *              d == 0: h_k = 0.  Otherwise r = (2 * gd) / d - 1;
 *              psi = r > 0 ? 2 / (1 + 1 / r) : 0;  h_k = (0.5 * psi) * d.
 *              (psi is van Leer's (r + |r|) / (1 + |r|) of the ratio r of the
 *              upwind-side to the face difference, written so that r = +inf
 *              gives 2 and a denormal r gives 0; the face value is the upwind
 *              cell's plus h_k.)  corr_i = sum_k F_k * h_k over those slots,
 *              from +0.  Boundary slots carry no correction: the inlet stays
 *              first-order.
 *   clamp      m_i, M_i start as phi_i and take, in slot order, v < m ? v : m
 *              and v > M ? v : M with v = phi_o on internal slots and v =
 *              inlet_value on inlet slots.
 *                t  = a_t * phi_i - corr_i;  lo = a_t * m_i;  hi = a_t * M_i
 *                t  = t < lo ? lo : (t > hi ? hi : t)
 *              (comparisons: a NaN t stays NaN and the advance returns
 *              CFD_ERR_DIVERGED as before).  b_i = t, then + c_k * inlet_value
 *              per inlet slot in slot order.  A cell counts as clamped when
 *              t < lo or t > hi held.
 * The bound: with v_i = b's t / a_t inside the range of phi_old over the cell,
 * its neighbours and the inlet, every Jacobi iterate (a_t v_i + sum_k c_k
 * phi_j + inlet terms) / diag_i is a convex combination with scheme 0's
 * weights of values inside that range, converged or not, so a dye in [0, 1]
 * stays there up to the same rounding as under scheme 0 (method 1 keeps its
 * own, wider bound).  The correction is not repeated: one pass per advance.  */
typedef struct cfd_scalar_scheme {
  int32_t scheme;          /* 0 upwind, 1 limited linear (van Leer) */
  int32_t reserved[3];
} cfd_scalar_scheme;
typedef struct cfd_scalar_scheme_stats {
  int32_t scheme;          /* of the last cfd_scalar_advance, this field */
  uint32_t clamped_cells;  /* cells whose t the clamp changed in it; 0 under scheme 0 */
  int32_t reserved[2];
} cfd_scalar_scheme_stats;
void cfd_scalar_scheme_default(cfd_scalar_scheme* cfg); /* scheme 0; null ignored */
/* Takes effect at the next cfd_scalar_advance.  CFD_ERR_INVALID: scalars not
 * enabled, a bad field index, a scheme other than 0 or 1, a distributed
 * handle.  cfd_scalars_enable resets every field to scheme 0.               */
cfd_status cfd_set_scalar_scheme(cfd_solver* s, int32_t field, const cfd_scalar_scheme* cfg);
cfd_status cfd_scalar_scheme_stats_get(cfd_solver* s, int32_t field, cfd_scalar_scheme_stats* out);

/* Wall conditions, sources and the wall-flux diagnostic of one scalar field.
 * By default every wall face is adiabatic (c_k = 0 above) and there is no
 * source, so a temperature can only enter through the inlet.  Per field, one
 * box of wall faces can carry a fixed value (a heated obstacle) or a fixed
 * flux, one box of cells a uniform source, and the rate at which the selected
 * faces give density * phi to the fluid can be read: the scalar counterpart of
 * cfd_flow_diag's wall force.  Everything is per field and opt-in: a field with
 * kind 0 and rate 0 launches the kernels above with the same arguments and
 * produces the same bits, a handle that never selects anything allocates
 * nothing new on the device, and cfd_step launches none of it in any case.
 * (On the host every one-GPU handle keeps the mesh view's f64 cell centres
 * from its creation, 16 bytes per cell, for the source box: the view itself
 * is not kept.)  The first
 * selection of a field that marks a face or a cell allocates its selection
 * image (one 32-bit word per cell), the first cfd_scalar_wall_flux_get with
 * faces to sum a few unit partials; cfd_scalars_enable frees both and resets
 * every field to kind 0 and rate 0.  One wall box and kind and one source box
 * per field, constant in time.  One GPU only, as the scalars are; checkpoints
 * neither store nor touch any of it.
 *
 * Arithmetic of wall conditions and sources.  All f32, one rounding per
 * operation (nothing fused), every sum left to right in face-slot order; rd =
 * density * D_f, A_k the face area, d_k the distance from the cell centre to
 * the face centre, the one the momentum wall diffusion uses.  Only wall faces
 * (boundary type 3) can be selected; an unselected wall stays adiabatic.
 *   kind 1     (fixed value) on a selected slot c_k = rd * A_k / d_k -- no
 *              convective part, a wall carries no flux -- and, at the slot's
 *              place in the loop, diag += c_k and b += c_k * value, as an inlet
 *              slot does with inlet_value.  The Jacobi row skips boundary slots
 *              as before.
 *   kind 2     (fixed flux) on a selected slot c_k = 0 and, at the slot's place,
 *              b += value * A_k: value is the flux of density * phi per unit
 *              area INTO the fluid.
 *   source     in a selected cell, after the slot loop, b += vol_i * rate: rate
 *              is density * phi per unit volume and time.
 *   scheme 1   gradient: the face value of a selected kind-1 slot is value
 *              (every other wall slot: phi_i as before).  clamp: m_i and M_i also
 *              take v = value on a selected kind-1 slot, at the slot's place, as
 *              they take inlet_value on an inlet slot.  The clamp applies to
 *              a_t * phi_i - corr_i as before; b_i = t, then one pass in
 *              ascending slot order over the inlet slots and the selected wall
 *              slots adds c_k * inlet_value (inlet), c_k * value (kind 1, c_k
 *              formed again by the same expression) or value * A_k (kind 2);
 *              the source term comes last.
 * The bound.  With kind 1 alone every Jacobi iterate is still a convex
 * combination: the weights gain c_k / diag_i on `value`.  A dye in [0, 1] with
 * value in [0, 1] keeps its bound with scheme 0's rounding allowance under
 * schemes 0 and 1, and method 1 keeps its own tol * max_i(diag_i / a_t,i).
 * Kind 2 and sources add to b without a matching weight: they are outside the
 * bound by construction (a heated wall heats).
 *   wall flux  per cell, in f64, in slot order over its selected slots, from +0:
 *                kind 1   flux += (double)c_k * ((double)value - (double)phi_i),
 *                         c_k the f32 coefficient above
 *                kind 2   flux += (double)value * (double)A_k
 *                area += (double)A_k;  phi_area += (double)A_k * (double)phi_i
 *              and the three per-cell terms (+0 in a cell without a selected
 *              slot) summed over the cells in the canonical order, the tree of
 *              cfd_scalar_stats.integral.  phi is the current field and density
 *              and D_f the current ones: right after an advance, flux is the
 *              implicit wall term of that advance, so that
 *                (density / dt) (I_new - I_old) = inlet + outlet + defect - clamp
 *                                                 + flux + rate * (volume of the source cells)
 *              closes to the rounding of the rows.                            */
typedef struct cfd_scalar_wall {
  int32_t kind;            /* 0 adiabatic (the default), 1 fixed value, 2 fixed flux */
  float value;             /* kind 1: phi on the selected faces; kind 2: the flux into the fluid */
  double x0, y0, x1, y1;   /* closed box over the f64 wall-face centres, cfd_set_force_region's rule; x1 < x0: none */
} cfd_scalar_wall;
typedef struct cfd_scalar_source {
  float rate;              /* density * phi per unit volume and time; 0: none */
  int32_t reserved;
  double x0, y0, x1, y1;   /* closed box over the f64 cell centres; x1 < x0: none */
} cfd_scalar_source;
typedef struct cfd_scalar_wall_flux {
  double flux;             /* density * phi per unit time entering the fluid through the selected faces */
  double area;             /* sum of their areas */
  double phi_area;         /* sum of A_k * phi_i over them (mean adjacent value = phi_area / area) */
  uint32_t faces;          /* wall faces in the field's box */
  int32_t kind;            /* the field's wall kind */
} cfd_scalar_wall_flux;
/* Both setters take effect at the next cfd_scalar_advance; *count (optional)
 * receives the wall faces / cells in the box.  Kind 0, a box without a wall
 * face, rate 0 or a box without a cell put the field back on the plain
 * kernels.  CFD_ERR_INVALID: scalars not enabled, a bad field index, a kind
 * outside 0..2, a value or rate that is not finite, a distributed handle, or
 * (kind 1 or 2) a selected wall face at slot 31 or above of its cell: the
 * selection keeps a cell's slots in 31 bits, as scheme 1 keeps 32.  A refused
 * call changes nothing.                                                      */
cfd_status cfd_set_scalar_wall(cfd_solver* s, int32_t field, const cfd_scalar_wall* cfg, uint32_t* faces);
cfd_status cfd_set_scalar_source(cfd_solver* s, int32_t field, const cfd_scalar_source* cfg, uint32_t* cells);
/* The wall-flux sums of the field as it stands.  Kind 0 or no selected face:
 * zeros (faces and kind filled in), nothing launched.                        */
cfd_status cfd_scalar_wall_flux_get(cfd_solver* s, int32_t field, cfd_scalar_wall_flux* out);

/* Boussinesq buoyancy: a scalar field drives the flow.  Each enabled field f
 * may carry an expansion coefficient beta_f and a reference value ref_f, the
 * solver one gravity vector g = (g_x, g_y), e.g. (0, -9.81); the momentum
 * equation gains the force per unit volume
 *   -density * sum_f beta_f (phi_f - ref_f) * g.
 * Opt-in: while every beta is 0 or g = (0, 0) (the defaults) cfd_step launches
 * the assembly kernel it always launched, with the same arguments, and
 * produces the same bits; otherwise the assembly runs in its buoyant form,
 * which reads 4 more bytes per cell and driving field.
 * The coupling is explicit: a cfd_step reads the fields as they stand when it
 * is called, every Picard iteration of that step the same values, and the
 * caller alternates cfd_step and cfd_scalar_advance as before.  The splitting
 * is first order in dt.
 *
 * Arithmetic of buoyancy.  All f32, one rounding per operation (nothing
 * fused), per owned cell i, after the face loop of the assembly and before its
 * stores, the fields in ascending index order and only those with beta_f != 0:
 *   d  = phi_f[i] - ref_f
 *   fb = (vol_i * density) * (beta_f * d)
 *   rhs_u = rhs_u - fb * g_x
 *   rhs_v = rhs_v - fb * g_y
 * Nothing else changes: not the matrix, rhs_p, the diagonal inverses, nor the
 * Rhie-Chow face flux of prepare_coupled.  The last is a known inconsistency
 * of collocated schemes: the face flux does not see the body force, so a sharp
 * front of phi leaves a small spurious divergence next to it
 * (cfd_flow_diag.max_divergence shows it).
 * The pressure then carries the hydrostatic part: cfd_flow_diag.force_pressure
 * contains the buoyant lift of the selected walls.
 *   body force  cfd_buoyancy_force_get: the counterpart of cfd_flow_diag's wall
 *              force, the term that closes a momentum budget.  Per cell, in
 *              f64, from +0 over the driving fields in field order:
 *                m   = (((double)vol_i * (double)density) * (double)beta_f)
 *                      * ((double)phi_f[i] - (double)ref_f)
 *                t_x = t_x - m * (double)g_x;  t_y = t_y - m * (double)g_y
 *              and the two per-cell terms summed over the cells in the
 *              canonical order, the tree of cfd_scalar_stats.integral.  phi and
 *              density are the current ones.  Buoyancy off (no beta != 0, or g =
 *              (0, 0)): (+0, +0), nothing launched.
 * cfd_scalars_enable (0, or a re-enable) clears every beta and ref; g stays.
 * Checkpoints do not store any of it (the file format and its version are
 * unchanged): a resumed run re-applies cfd_set_scalar_buoyancy, cfd_set_gravity
 * and cfd_set_scalar.  One GPU only, as the scalars are.                      */
typedef struct cfd_buoyancy {
  float gx, gy;
  int32_t fields;          /* enabled scalar fields */
  int32_t active;          /* 1: the next cfd_step assembles in the buoyant form */
  float beta[4];           /* 0 beyond `fields` */
  float ref[4];
} cfd_buoyancy;
typedef struct cfd_buoyancy_force {
  double force[2];         /* sum over the cells of -vol density sum_f beta_f (phi_f - ref_f) g */
  uint32_t fields;         /* driving fields (beta != 0) */
  uint32_t reserved;
} cfd_buoyancy_force;
/* Both setters take effect at the next cfd_step.  CFD_ERR_INVALID: a beta,
 * ref or g that is not finite, a distributed handle, and for the field setter
 * scalars not enabled or a bad field index.  A refused call changes nothing. */
cfd_status cfd_set_scalar_buoyancy(cfd_solver* s, int32_t field, float beta, float ref);
cfd_status cfd_set_gravity(cfd_solver* s, float gx, float gy);
/* The settings back; never fails on a valid handle.                          */
cfd_status cfd_buoyancy_get(const cfd_solver* s, cfd_buoyancy* out);
/* CFD_ERR_INVALID: scalars not enabled, a distributed handle.                */
cfd_status cfd_buoyancy_force_get(cfd_solver* s, cfd_buoyancy_force* out);

/* ------------------------------------------------------------------------ */
/* Prescribed boundary velocities: inlet profiles and moving walls.  Without
 * them the flow has one boundary velocity, inlet_velocity * ramp along +x on
 * every inlet face, and every wall is at rest.  cfd_set_boundary_velocity gives
 * a chosen set of inlet (1) and wall (3) boundary faces a velocity vector of
 * their own: a parabolic or pulsatile inlet, a rotating cylinder, a moving
 * belt.  Opt-in: with an empty selection (the default) cfd_step launches the
 * kernels it always launched, with the same arguments, and produces the same
 * bits; otherwise prepare_coupled, the assembly and the flow diagnostics run in
 * their BCV forms, which read 4 more bytes per cell and a compact table (one
 * row per cell with a selected face, O(sqrt N) rows) inside the boundary
 * branches only.  Walls stay impermeable: for a wall face the host removes the
 * normal component (v . n) n / (n . n) in f64 before it rounds the vector to
 * f32; cfd_boundary_velocity.max_normal_removed reports the largest |v . n| /
 * |n| removed since the selection was last empty.
 *
 * Arithmetic of boundary velocities.  All f32, one rounding per operation
 * (nothing fused).  For a selected slot with the uploaded (bx, by), in every
 * kernel that uses it:
 *   g   = scale * ramp     ramp = smoothstep(0, ramp_time, time) of the step,
 *                          scale = inlet_scale on an inlet slot, wall_scale on
 *                          a wall slot
 *   ubx = bx * g;  uby = by * g
 * prepare_coupled, selected inlet slot:
 *   flux = density * (ubx * nfx + uby * nfy) * area      (nf: the flux normal)
 *   face value of the velocity gradients: vfu = ubx, vfv = uby
 * prepare_coupled, selected wall slot: flux (0) and the diagonal (+ diff_coeff)
 *   are unchanged; vfu = ubx, vfv = uby.
 * assembly, selected inlet slot: the plain inlet branch with this ubx, and
 *   with uby where it has the literal 0, each operation at the slot's place in
 *   the face loop:
 *     diag += diff_coeff;  rhs_u += diff_coeff * ubx;  rhs_v += diff_coeff * uby
 *     flux > 0: diag += flux;  else rhs_u -= flux * ubx;  rhs_v -= flux * uby
 *     flux_bc = (ubx * nx + uby * ny) * area;  rhs_p -= flux_bc
 * assembly, selected wall slot: the plain wall branch (diag += diff_coeff, the
 *   pressure-gradient sums), then
 *     rhs_u += diff_coeff * ubx;  rhs_v += diff_coeff * uby
 * An unselected boundary slot keeps the plain arithmetic exactly.  d_p is
 * unchanged: the Rhie-Chow flux does not see a wall's tangential motion.
 * Flow diagnostics (cfd_flow_diagnostics, cfd_get_derived, the renderer's
 * vorticity, the monitor): the face value follows prepare_coupled; the viscous
 * force of a selected wall face of the force region is, in f64,
 *   viscosity * ((double)u - (double)ubx) * area / dist   (and v, uby)
 * in place of viscosity * u * area / dist.
 * cfd_wall_motion_get: over the wall faces of the force region
 * (cfd_set_force_region), per cell in f64 in ascending slot order, with F_p =
 * p n area and F_v as above (the forces of the fluid on the wall, as
 * cfd_flow_diag forms them) and r = (f64 face centre) - (x0, y0):
 *   torque_pressure += r_x F_py - r_y F_px
 *   torque_viscous  += r_x F_vy - r_y F_vx
 *   power           -= (F_px + F_vx) * ubx + (F_py + F_vy) * uby   selected faces only
 * each summed over the cells in the canonical order.  power is what the
 * selected moving walls of the region deliver to the fluid, -sum F_on_wall .
 * u_wall.  An empty region: zeros, nothing launched.
 * The scales are kernel arguments of prepare_coupled and the assembly, which a
 * step launches itself also when the Krylov iteration replays a captured graph
 * (cfd_graph_enable): a change takes effect at the next cfd_step.
 * Checkpoints do not store the selection or the scales (the file format and its
 * version are unchanged): a resumed run re-applies them.  One GPU only, and not
 * together with flag 2 of cfd_debug_reference_semantics.                     */
typedef struct cfd_boundary_velocity {
  uint32_t inlet_faces;      /* selected inlet faces */
  uint32_t wall_faces;       /* selected wall faces */
  float inlet_scale;
  float wall_scale;
  int32_t active;            /* 1: the next cfd_step runs the BCV forms */
  int32_t reserved;
  double max_normal_removed; /* largest |v . n| / |n| removed from a wall entry */
} cfd_boundary_velocity;
typedef struct cfd_wall_motion {
  double torque_pressure;    /* about (x0, y0), of the pressure force of the fluid on the region's walls */
  double torque_viscous;     /* ... of the viscous force */
  double power;              /* delivered to the fluid by the region's selected walls */
  uint32_t region_faces;     /* wall faces of the force region */
  uint32_t moving_faces;     /* of these, selected ones */
} cfd_wall_motion;
/* face_ids: global face indices, each an inlet (1) or wall (3) boundary face;
 * vx, vy: the f32 velocity of each.  A later entry (or call) replaces an earlier
 * one of the same face; n == 0 clears the whole selection (the pointers may be
 * null).  *selected (optional) = faces selected afterwards.  CFD_ERR_INVALID: a
 * face that is no inlet or wall boundary face, a velocity that is not finite, a
 * distributed handle, reference semantics with flag 2.  A refused call changes
 * nothing.  Takes effect at the next cfd_step.                               */
cfd_status cfd_set_boundary_velocity(cfd_solver* s, uint32_t n, const uint32_t* face_ids, const float* vx,
                                     const float* vy, uint32_t* selected);
/* Two factors (default 1, 1) applied on the device: a pulsatile inlet or an
 * oscillating rotation needs no new upload.  They stay over a cleared selection. */
cfd_status cfd_set_boundary_velocity_scale(cfd_solver* s, float inlet_scale, float wall_scale);
/* The settings back; never fails on a valid handle.                          */
cfd_status cfd_boundary_velocity_get(const cfd_solver* s, cfd_boundary_velocity* out);
/* Read-only.  CFD_ERR_INVALID: a distributed handle, x0 or y0 not finite.     */
cfd_status cfd_wall_motion_get(cfd_solver* s, double x0, double y0, cfd_wall_motion* out);

/* ------------------------------------------------------------------------ */
/* Variable viscosity: a viscosity per cell.  Without it the fluid has one
 * viscosity, cfd_constants::viscosity, in every face's diffusion coefficient.
 * cfd_set_viscosity_field gives every cell a viscosity of its own: the
 * mechanism a generalised Newtonian fluid (power law, Carreau), an eddy
 * viscosity or a temperature-dependent viscosity needs.  The caller uploads a
 * field of its own, once or before every step, or sets one of the models
 * below (cfd_set_viscosity_model), which the device evaluates every step.
 * Opt-in: without a field (the default, and again after a clear) cfd_step
 * launches the kernels it always launched, with the same arguments, and
 * produces the same bits; with one, prepare_coupled, the assembly, the flow
 * diagnostics, cfd_wall_motion_get and the surface run in their VISC forms,
 * which read one more coalesced 4-byte value per cell and gather one 4-byte
 * value per interior face slot, beside the neighbour's velocity.
 *
 * Arithmetic of variable viscosity.  All f32, one rounding per operation
 * (nothing fused).  With the uploaded mu[N], for face slot k of cell i whose
 * neighbour across the face is cell o:
 *   interior slot   mu_f = 0.5f * (mu[i] + mu[o])
 *   boundary slot   mu_f = mu[i]
 * The arithmetic mean is commutative in floating point: both cells of a face
 * form the same bits, so the diffusion part of the matrix stays symmetric bit
 * for bit.  mu_f replaces cfd_constants::viscosity and nothing else: in
 * prepare_coupled (the diagonal that gives d_p) and in the assembly (the
 * diagonal, the off-diagonal entry -diff_coeff + min(flux, 0), the boundary
 * terms diff_coeff * ub)
 *   diff_coeff = mu_f * area / dist
 * with each kernel's own distance as before: |centre - other centre| (|centre -
 * face centre| on a boundary slot) in prepare_coupled, max(|d . n|, 1e-6) in
 * the assembly.  A uniform field equal to cfd_constants::viscosity gives the
 * plain kernels' bits: 0.5f * (m + m) == m exactly.
 * Flow diagnostics, cfd_wall_motion_get and the surface channels 3 and 4: the
 * viscous force of a wall face of cell i is, in f64,
 *   (double)mu[i] * u_rel * area / dist
 * in place of (double)viscosity * u_rel * area / dist (u_rel: the velocity
 * relative to the wall, "Arithmetic of boundary velocities").
 * The pointer the kernels read stays the same while a field is set, and they
 * read its contents when they run: replacing the field between steps costs one
 * upload, also when the Krylov iteration replays a captured graph
 * (cfd_graph_enable); prepare_coupled and the assembly are launched by the step
 * itself.  The field takes effect at the next cfd_step.
 * Checkpoints do not store the field (the file format and its version are
 * unchanged): a resumed run sets it again.  One GPU only, and not together with
 * flags 1 or 2 of cfd_debug_reference_semantics.                             */
/* n == num_cells: enables the field or replaces its values; n == 0 clears it
 * (mu may be null).  CFD_ERR_INVALID: any other n, a value that is not finite
 * or not > 0, a distributed handle, reference semantics with flag 1 or 2.  A
 * refused call changes nothing.                                              */
cfd_status cfd_set_viscosity_field(cfd_solver* s, const float* mu, uint32_t n);
/* out[num_cells]: the field the next cfd_step will read (and, unless it was
 * replaced since, the last one did).  CFD_ERR_INVALID: no field is set.       */
cfd_status cfd_get_viscosity_field(cfd_solver* s, float* out);
/* The viscosity models: generalised Newtonian fluids evaluated on the device.
 * With a model set, cfd_step evaluates it once, before the first Picard
 * iteration, from the velocity the step starts from, and the whole step reads
 * that field (first-order lagging, the splitting stance of buoyancy).
 *
 * Arithmetic of the viscosity models.  Per cell, the Green-Gauss gradients
 * (ux, uy) of u and (vx, vy) of v of the CURRENT velocity exactly as
 * prepare_coupled forms them (its face values, those of "Arithmetic of
 * boundary velocities" with a selection on; not the gradients a previous step
 * left), so the field is a function of the state alone.  Then, every operation
 * one rounding in this order, the parameters widened from f32:
 *   f32  gdot = sqrtf(2*(ux*ux) + 2*(vy*vy) + (uy+vx)*(uy+vx))
 *   f64  power law (kind 1)  m = K * pow_det(max(gdot, gamma_min), n - 1)
 *   f64  Carreau   (kind 2)  m = mu_inf + (mu0 - mu_inf) * pow_det(1 + (lambda*gdot)*(lambda*gdot), (n - 1) / 2)
 *   f32  mu = (float) min(max(m, mu_min), mu_max)
 * pow_det(x, y) = x^y from IEEE + - * /, frexp, ldexp and rint alone, the same
 * bits on the host and the device (csrc/hip/pow_det.hpp states the series, the
 * term counts and the error bound (16 + 8 |y ln x|) 2^-53).  A cell counts as
 * clamped below when m < mu_min and above when m > mu_max.
 * cfd_set_viscosity_model enables the field (evaluating the model on the
 * current state at once); cfd_set_viscosity_field and clearing the field clear
 * the model; kind 0 clears the model and leaves the field as it stands.
 * Checkpoints store neither: a resumed run sets the model again, and because
 * the field is a function of the state its next step has the bits of the
 * uninterrupted run.  One GPU only; not with reference-semantics flags 1, 2.   */
typedef struct cfd_viscosity_model {
  int32_t kind;     /* 0 none, 1 power law, 2 Carreau */
  float K, n;       /* power law: consistency K > 0, index n; Carreau reads n too */
  float gamma_min;  /* power law: > 0, the shear rate below which the law is cut off */
  float mu0, mu_inf, lambda; /* Carreau: mu0 > 0, mu_inf >= 0, lambda > 0 */
  float mu_min, mu_max;      /* 0 < mu_min <= mu_max, both finite */
} cfd_viscosity_model;
typedef struct cfd_viscosity_stats {
  float mu_min, mu_max;     /* over the cells, of the last evaluation */
  uint32_t clamped_below, clamped_above;
} cfd_viscosity_stats;
/* CFD_ERR_INVALID: an unknown kind, a parameter of the chosen kind that is not
 * finite or outside the ranges above, mu_min > mu_max, a distributed handle,
 * reference semantics with flag 1 or 2.  A refused call changes nothing.      */
cfd_status cfd_set_viscosity_model(cfd_solver* s, const cfd_viscosity_model* model);
/* Evaluates the model on the current state now (cfd_step does it by itself).
 * CFD_ERR_INVALID for this and the two below: no model is set.                */
cfd_status cfd_viscosity_evaluate(cfd_solver* s);
/* out[num_cells]: gdot of the last evaluation.                               */
cfd_status cfd_get_shear_rate(cfd_solver* s, float* out);
cfd_status cfd_viscosity_stats_get(cfd_solver* s, cfd_viscosity_stats* out);
/* Test-only: out[i] = pow_det(x[i], y[i]) by the host copy of csrc/hip/pow_det.hpp. */
cfd_status cfd_debug_pow_det(const double* x, const double* y, double* out, uint32_t n);

/* ------------------------------------------------------------------------ */
/* Volume penalisation: a term in the momentum equation that acts inside the
 * fluid.  Every cell gets a linear drag towards a target velocity,
 *   rho du/dt + ... = ... - s (u - u_t),     s = sigma + forch |u|
 * sigma large and u_t = 0: the cell behaves as a solid (Brinkman
 * penalisation); sigma moderate: a Darcy porous medium, forch adding the
 * Forchheimer quadratic drag; u_t != 0: a body that moves or rotates through
 * the fixed mesh; sigma rising towards the outlet: a sponge layer.  The term is
 * diagonal and implicit.  Opt-in: without a field (the default, and again after
 * a clear) cfd_step launches the kernels it always launched, with the same
 * arguments, and produces the same bits; with one, prepare_coupled and the
 * assembly run in their PEN forms, which read 4 more bytes per cell (sigma), 4
 * more with forch and, in the assembly, 8 more with a target, all coalesced.
 *
 * Arithmetic of volume penalisation.  All f32, one rounding per operation
 * (nothing fused), in this order, for cell i; uc = u[i] of the current iterate,
 * the velocity both kernels already load:
 *   s   = sigma[i]                                              forch null
 *   s   = sigma[i] + forch[i] * sqrtf(uc.x*uc.x + uc.y*uc.y)    forch set
 *   pen = vol[i] * s
 *   prepare_coupled: diag_coeff += pen    after the face loop, before d_p = vol / diag_coeff
 *   assembly:        diag_uv    += pen    after the face loop and the buoyancy term
 *                    rhs_u      += pen * (target_scale * target[i].x)
 *                    rhs_v      += pen * (target_scale * target[i].y)
 * With a null target nothing is added to the right-hand side (not even +0).
 * Because forch reads the iterate, the quadratic drag is re-evaluated at every
 * Picard iteration at no extra cost; prepare_coupled and the assembly of one
 * iteration read the same state, so d_p and the momentum diagonal agree, and
 * the Rhie-Chow flux and the pressure Laplacian see the drag through d_p with
 * no change of their own.  Nothing else in either kernel changes: no
 * off-diagonal momentum coefficient changes bits.  sigma == 0 everywhere with
 * null forch and target gives the plain step's bits: the diagonals are
 * positive and x + 0.0f == x (no -0 exception is known: neither diagonal can
 * be -0, a sum that starts from the positive time coefficient).
 * The pointers the kernels read stay the same while a field is set, and they
 * read the contents when they run: replacing the field between steps is one
 * upload, also when the Krylov iteration replays a captured graph;
 * target_scale is a kernel argument, so an oscillating body costs no upload.
 *
 * The limit on vol * sigma.  The pressure row of cell i has the diagonal
 *   sdiag_i = sum over its interior and outlet slots of density * dp_f * area / dist
 * with dp_f = lambda d_p[i] + (1 - lambda) d_p[other], lambda in [0, 1] (d_p[i]
 * on an outlet slot), and the preconditioner takes 1 / sdiag_i only when
 * |sdiag_i| > 1e-14, else 0.  So sdiag_i >= density * G_i * min d_p, with G_i
 * the sum of area / dist over those slots, the minimum over cell i and its
 * neighbours.  d_p[j] = vol_j / (B_j + pen_j), B_j the plain diagonal; where the
 * penalty dominates (pen_j >= B_j) d_p[j] >= vol_j / (2 pen_j).  With pen_j <= L
 * everywhere, the penalty alone cannot push a pressure diagonal under the
 * threshold when  density * min(G) * min(vol) / (2 L) > 1e-14.  With a further
 * factor 2 of margin, on this handle's mesh and with the density as it stands
 * at the call,
 *   L = density * min_i(G_i) * min_i(vol_i) / 4e-14
 * and cfd_set_penalty refuses a field with vol[i] * sigma[i] > L for any cell
 * (cfd_penalty_info::max_vol_sigma reports L).  On a uniform mesh of spacing h
 * with density 1, G = 4 and L = 1e14 h^2, that is sigma <= 1e14.  The limit is
 * on the uploaded sigma: the Forchheimer part forch |u| is part of the state and
 * is not bounded by it; lowering the density afterwards lowers the margin in
 * proportion.  Where B_j dominates, d_p is within a factor 2 of the plain
 * solver's and the penalty is not what makes it small.
 *
 * The force diagnostic.  cfd_penalty_force_get makes one read-only pass over
 * the current state, per cell in f64 (every f32 value widened first, one
 * rounding per operation):
 *   s  = sigma + forch * sqrt(ux*ux + uy*uy)       (forch null: s = sigma)
 *   m  = vol * s;   tx = target_scale * target.x,  ty = target_scale * target.y   (null: 0, 0)
 *   fx = m * (ux - tx);   fy = m * (uy - ty)
 *   F = sum (fx, fy)                    the force of the fluid on the penalised medium
 *   tau = sum rx * fy - ry * fx         r = the f64 cell centre - (cx, cy)
 *   P = sum fx * tx + fy * ty           the rate of work of that force on the moving medium
 *                                       (negative where the body drives the fluid: the body delivers -P)
 *   n = cells with s > 0
 * each sum in the canonical leaf / chunk / segment / total order of the other
 * f64 diagnostics, so the bits do not depend on the scheduling.  With a box the
 * sums run over the cells whose f64 centre lies in the closed box (the force
 * region's rule: x0 <= x <= x1 and y0 <= y <= y1, none for x1 < x0), so two
 * bodies can be read separately.  It is the drag and lift of an immersed body,
 * the counterpart of cfd_flow_diagnostics' wall force, and the term that closes
 * a momentum budget beside it and cfd_buoyancy_force_get.
 * Checkpoints store none of this (the file format and its version are
 * unchanged): a resumed run sets the field and the scale again.  One GPU only,
 * and not together with flags 1 or 2 of cfd_debug_reference_semantics.       */
typedef struct cfd_penalty_info {
  int32_t active;        /* a field is set */
  int32_t has_forch, has_target;
  float target_scale;    /* 1 until cfd_set_penalty_scale */
  double max_vol_sigma;  /* L above, with the density as it stands */
} cfd_penalty_info;
typedef struct cfd_penalty_force {
  double force[2];
  double torque;
  double power;
  uint32_t cells;        /* with s > 0 (inside the box) */
  uint32_t reserved;
} cfd_penalty_force;
/* sigma[n], forch[n] or null, target[2 n] (x, y per cell) or null.
 * n == num_cells: sets or replaces the field (one upload; the device pointers
 * stay); n == 0 clears it (the pointers may be null).  Every value is checked
 * before anything changes.  CFD_ERR_INVALID: any other n; a value that is not
 * finite; a negative sigma or forch; max(vol) * max(sigma) not finite in f32;
 * vol[i] * sigma[i] above the limit L; a distributed handle; reference
 * semantics with flag 1 or 2.  A refused call changes nothing.                */
cfd_status cfd_set_penalty(cfd_solver* s, const float* sigma, const float* forch, const float* target, uint32_t n);
/* target_scale (finite), a kernel argument of the next launches; may be set
 * before a field; survives a clear.                                           */
cfd_status cfd_set_penalty_scale(cfd_solver* s, float target_scale);
/* info and the arrays are optional (null: skipped).  A read: info is answered on
 * every handle, also a distributed one and in the reference-semantics modes,
 * where no field can be set and active is 0.  CFD_ERR_INVALID: an array asked
 * for without a field, forch or target asked for when none is set.            */
cfd_status cfd_get_penalty(cfd_solver* s, cfd_penalty_info* info, float* sigma, float* forch, float* target);
/* box: {x0, y0, x1, y1} or null (every cell).  Read-only.  CFD_ERR_INVALID: no
 * field is set, cx or cy not finite, a NaN in the box, a distributed handle.   */
cfd_status cfd_penalty_force_get(cfd_solver* s, double cx, double cy, const double* box, cfd_penalty_force* out);

/* ------------------------------------------------------------------------ */
/* Frames on the device: a cell field as an H x W RGBA8 image, the headless
 * form of the reference's renderer (src/ui/cfd_renderer.rs fan-triangulates
 * every cell, cfd_mesh_shader.wgsl colours each fan by the cell's value).  The
 * picture is a pure function of the state, the cell polygons, a view box and a
 * value range.  Opt-in and read-only: a handle that never calls
 * cfd_render_set_polygons allocates and launches nothing new, cfd_step
 * launches none of it in any case, and nothing a step reads is written.  One
 * GPU only: handles of cfd_solver_create_dist* and members of a group of more
 * than one rank return CFD_ERR_INVALID.  Checkpoints store none of it: the
 * polygons and the view are not state.  Not built: the reference's mesh-line
 * overlay (fs_solid), other colour maps, anti-aliasing.
 *
 * The picture.  All f32, one rounding per operation (nothing fused).
 *   polygons   cfd_mesh_view has no vertices; the caller uploads the mesh's
 *              vertex arrays and the CCW cell polygons (cfd_mesh_get_vertices,
 *              cfd_mesh_get_topology).  Vertices are rounded to f32 once.  Cell
 *              c is the union of its fan triangles (v_0, v_i, v_i+1), 1 <= i <=
 *              n - 2 (build_mesh_vertices); fewer than 3 vertices: nothing.
 *   view       a world box [x0, x1] x [y0, y1], each bound rounded to f32 once,
 *              x1 > x0 and y1 > y0 after the rounding; the default is the
 *              bounding box of the polygons' vertices (compute_bounds), with no
 *              aspect correction.  1 <= W, H <= 8192.
 *                dx = (x1 - x0) / W;  dy = (y1 - y0) / H
 *              (both must come out > 0).  Pixel (row j, column i) has the centre
 *                px = x0 + (i + 0.5) * dx;  py = y1 - (j + 0.5) * dy
 *              with i, j and the 0.5 exact in f32: row 0 is the top.
 *   edges      the edge function of an edge between vertex INDICES a < b is
 *                E(p) = (xb - xa) * (py - ya) - (yb - ya) * (px - xa);
 *              an edge traversed from b to a uses -E, so the two cells that
 *              share an edge see exact negations and the closed tests below
 *              leave no crack between them.  (a == b: E as written, which is 0.)
 *   triangles  a triangle (v_0, v_i, v_i+1) has the edge values e_1, e_2, e_3 of
 *              its edges v_0 -> v_i, v_i -> v_i+1, v_i+1 -> v_0.  It owns p if
 *              all three are >= 0, or if all three are <= 0 (both windings are
 *              drawn, as a rasteriser without culling does).  A triangle whose
 *              e_1 at its own third vertex v_i+1 is 0 has no area and is skipped.
 *   candidates a cell is tested against the pixels of its pixel box only.  With
 *              [mnx, mxx] x [mny, mxy] the bounds of its vertices (a NaN
 *              coordinate is ignored by the comparisons),
 *                i from floor((mnx - x0) / dx - 0.5) to ceil((mxx - x0) / dx - 0.5)
 *                j from floor((y1 - mxy) / dy - 0.5) to ceil((y1 - mny) / dy - 0.5)
 *              clipped to the image: every centre inside the bounds and up to
 *              one more pixel per side.  It is part of the definition, so that
 *              the map does not depend on how an implementation culls.
 *   owner      a pixel belongs to the LARGEST cell index among the cells that
 *              own its centre, to none (UINT32_MAX) if there are none.  That
 *              rule makes the map independent of scheduling.
 *   value      field 0 speed sqrt(u.x * u.x + u.y * u.y) (the shader's mode 1;
 *              the f32 square root correctly rounded), 1 u.x, 2 u.y, 3 p,
 *              4 vorticity and 5 divergence (cfd_get_derived's f32 values),
 *              6 scalar field `scalar_index`.
 *   colour     cfd_mesh_shader.wgsl:60-93; every pixel of a fan has the same
 *              cell, so the interpolated value is the cell's value.
 *                r = hi - lo;  safe = |r| < 1e-10 ? 1 : r;  q = (val - lo) / safe
 *              (a true division).  q is NaN (a NaN value, or a range that makes
 *              one): the pixel is (0, 0, 0, 255).  Otherwise t = q < 0 ? 0 :
 *              (q > 1 ? 1 : q) and
 *                t < 0.5:    s = t * 2;          (R, G, B) = (0, s, 1 - s)
 *                otherwise:  s = (t - 0.5) * 2;  (R, G, B) = (s, 1 - s, 0)
 *              each channel the byte (uint8)(c * 255 + 0.5), alpha 255.  A pixel
 *              without an owner is (0, 0, 0, 0).  (The reference leaves the
 *              8-bit rounding to its render target; this one is stated here.)
 *   auto range with no range given, lo and hi are the minimum and the maximum of
 *              the field over ALL cells, on or off the image, NaN cells ignored
 *              (what app.rs does on the host before it draws), found on the
 *              device over cfd_scalar_stats' order-preserving keys (so -0 <
 *              +0).  No cell without a NaN: (0, 1).  The range used is returned.
 * Bytes: rgba[4 * (j * W + i) + k], k = 0 R, 1 G, 2 B, 3 A.                   */
enum { CFD_RENDER_SPEED = 0, CFD_RENDER_UX = 1, CFD_RENDER_UY = 2, CFD_RENDER_P = 3, CFD_RENDER_VORTICITY = 4,
       CFD_RENDER_DIVERGENCE = 5, CFD_RENDER_SCALAR = 6 };
/* Uploads the polygons of the handle's N cells (the first call allocates the
 * renderer's own device memory) and drops the view.  num_vertices 0 releases
 * everything (the other arguments are ignored; later render calls return
 * CFD_ERR_INVALID).  CFD_ERR_INVALID: a distributed handle, a null array,
 * cell_vertex_offsets[0] != 0, offsets that decrease, cell_vertex_offsets[N]
 * >= 2^31, a vertex index >= num_vertices.  A refused call changes nothing.   */
cfd_status cfd_render_set_polygons(cfd_solver* s, uint32_t num_vertices, const double* vx, const double* vy,
                                   const uint32_t* cell_vertex_offsets /* [N + 1] */,
                                   const uint32_t* cell_vertices /* [cell_vertex_offsets[N]] */);
/* Builds the ownership map of a view: once per (polygons, view), not per
 * frame.  box = {x0, y0, x1, y1}; null: the polygons' bounds.  *covered
 * (optional) = the pixels that have an owner.  CFD_ERR_INVALID: no polygons,
 * a size outside 1..8192, a box that is not finite or empty after rounding; a
 * refused call leaves the handle without a view.                              */
cfd_status cfd_render_set_view(cfd_solver* s, int32_t width, int32_t height, const double box[4], uint32_t* covered);
/* One frame of the current state into rgba[H * W * 4].  range = {lo, hi};
 * null: the auto range.  used_range (optional) receives the range used.
 * CFD_ERR_INVALID: no polygons, no view, a field outside 0..6, field 6 with
 * scalars not enabled or a bad scalar_index.                                  */
cfd_status cfd_render(cfd_solver* s, int32_t field, int32_t scalar_index, const float range[2], uint8_t* rgba,
                      float used_range[2]);
/* The ownership map, out[j * W + i] = the owner or UINT32_MAX: for picking
 * ("which cell is under the cursor") and for tests.                           */
cfd_status cfd_render_owner_get(cfd_solver* s, uint32_t* out /* [H * W] */);

/* ------------------------------------------------------------------------ */
/* Tracer particles: a set of massless points that lives on the device, is
 * located in the mesh there and is carried face to face by the current
 * velocity field: pathlines, streaklines (re-seed a ring of slots at a rake
 * every step), residence times (the age).  Opt-in and read-only: a handle that
 * never calls cfd_particles_set_mesh allocates and launches nothing new,
 * cfd_step launches none of it in any case, and nothing a step reads is
 * written.  One GPU only: handles of cfd_solver_create_dist* and members of a
 * group of more than one rank return CFD_ERR_INVALID.  Checkpoints store none
 * of it: neither the mesh upload nor the particles are solver state; a caller
 * who resumes reads the particles with cfd_particles_get before and seeds them
 * again after.  Beyond the reference, which has no particles.
 *
 * The tracers.  All f32, one rounding per operation (nothing fused).
 *   geometry   as for the picture: vertices rounded to f32 once, and the edge
 *              function E of an edge between vertex INDICES a < b,
 *                E(q) = (xb - xa) * (qy - ya) - (yb - ya) * (qx - xa).
 *              Face slot k of cell c (the k-th entry of the cell's row of
 *              cell_faces) has the face's two vertices as a < b and a sign
 *              fixed at upload: the face's vertices are consecutive in the
 *              cell's CCW polygon, and
 *                g_k(q) = E(q) where the polygon runs a -> b, -E(q) where b -> a,
 *              so g_k >= 0 on the cell's side of the face's line.  The two
 *              cells of a face see exact negations: a point is never strictly
 *              outside both.
 *   bins       [bx0, bx1] x [by0, by1] = the f32 bounds of the polygons'
 *              vertices; nb = min(1024, ceil(sqrt(N))) bins per direction of
 *                sx = (bx1 - bx0) / nb;  sy = (by1 - by0) / nb
 *              (both must come out > 0).  bin(x) = floor((x - bx0) / sx) clamped
 *              to [0, nb - 1], a NaN to 0; likewise in y.  A cell is listed in
 *              every bin (i, j) with bin(mnx) <= i <= bin(mxx) and bin(mny) <= j
 *              <= bin(mxy) of its vertices' f32 bounds.
 *   locate     a point belongs to the LARGEST cell index among the listed
 *              cells of its bin whose fan triangles own it under the picture's
 *              closed test ("triangles" above, zero-area triangles skipped):
 *              the rule of cfd_render_owner_get for a pixel centre.  bin() is
 *              monotone and a point inside a fan triangle is inside the cell's
 *              bounds, so the bins change no answer.  No owner: OUTSIDE.
 *   advance    per ALIVE particle, independently of all others; u is the
 *              current state's velocity, frozen for the call.  Start: r = dt,
 *              c = the particle's cell, v = u[c], no excluded slot, hops = 0.
 *              Repeat:
 *                e = p + v * r                     (per component: one product, one sum)
 *                for each slot k < nface[c] but the excluded one, in order:
 *                  ge = g_k(e);  gp = g_k(p)
 *                  ha = v.x * (ya - p.y) - v.y * (xa - p.x);  hb likewise for b
 *                  candidate if ge < 0 and ((ha >= 0 and hb <= 0) or (ha <= 0
 *                  and hb >= 0)): the end point is beyond the face's line AND
 *                  the face's two vertices lie on opposite closed sides of the
 *                  path's line (real segments, not half-planes: cells with moved
 *                  hanging nodes are not convex, collinear faces share a line)
 *                  t_k = gp <= 0 ? 0 : gp / (gp - ge)
 *                the smallest t_k wins, ties to the lowest slot.
 *                no candidate, but some slot (not the excluded one) has ge < 0 and
 *                  the cell's fan triangles do not own e (locate's closed test):
 *                  a path along a face's line, as a wall slide that ends at the
 *                  face's vertex, can miss every segment by a rounding.  Then
 *                  every such slot is a candidate (half-planes), same t_k, same
 *                  choice.
 *                no candidate: p = e, age = age + r, done.
 *                hops == hop_cap: the particle stays where it is, the rest of r
 *                  is dropped (the age does not take it), it counts as capped,
 *                  done.  This bounds the work, also at a face where the two
 *                  cells' velocities point at each other.
 *                otherwise: s = r * t;  p = p + v * s;  age = age + s;
 *                  r = r - s;  hops = hops + 1; then by the slot's boundary type
 *                  internal  c = the slot's neighbour, v = u[c], no excluded slot
 *                  outlet    status EXITED_OUTLET, done: position and age stay
 *                  inlet     status EXITED_INLET, likewise
 *                  wall      contacts + 1;  dn = v.x * nx + v.y * ny;
 *                            v = (v.x - dn * nx, v.y - dn * ny) (the slot's
 *                            outward normal) until the particle leaves the cell
 *                            or the call ends; this slot is the excluded one
 *                            (a second wall of the same cell replaces it).
 *              The velocity is piecewise constant, so a path is straight inside
 *              a cell: exact in time for that field, first order in space.
 *   stamp      an ALIVE particle covers pixel
 *                i = floor((p.x - x0) / dx);  j = floor((y1 - p.y) / dy)
 *              of the current view (x0, y1, dx, dy of "view" above) if 0 <= i <
 *              W and 0 <= j < H, compared in f32.
 * Status values; cell is the particle's cell (ALIVE), the cell it left through
 * a boundary face (EXITED_*), UINT32_MAX otherwise.                           */
enum { CFD_PARTICLE_EMPTY = 0, CFD_PARTICLE_ALIVE = 1, CFD_PARTICLE_EXITED_OUTLET = 2, CFD_PARTICLE_EXITED_INLET = 3,
       CFD_PARTICLE_OUTSIDE = 4 };
typedef struct cfd_particle_config {
  int32_t hop_cap; /* face crossings per particle and advance: 1..65536; 0: the default 64 */
  int32_t reserved[3];
} cfd_particle_config;
void cfd_particle_config_default(cfd_particle_config* out);
/* Integer counts reduced on the device: independent of any order.             */
typedef struct cfd_particle_stats {
  uint64_t count[5];      /* slots per status; they sum to the capacity            */
  uint64_t wall_contacts; /* over all slots, since each was seeded                 */
  uint64_t hops_total;    /* face crossings of the last advance                    */
  uint64_t hops_max;      /* ... the most of one particle                          */
  uint64_t capped;        /* particles that hit hop_cap in the last advance        */
  uint64_t capacity;
} cfd_particle_stats;
/* Uploads the vertices, the CCW cell polygons and the two vertices of every
 * face (cfd_mesh_get_vertices, cfd_mesh_get_topology) into the module's own
 * device memory, with the per-slot vertex pairs and the bin grid built on the
 * host.  It frees the particle set of an earlier mesh.  num_vertices 0 releases
 * everything (the other arguments are ignored).  CFD_ERR_INVALID: what
 * cfd_render_set_polygons refuses, num_vertices >= 2^31, a polygon that is not
 * counter-clockwise, a face whose two vertices are equal, out of range or not
 * consecutive in the polygon of a cell that lists it, bounds that are empty or
 * not finite.  A refused call changes nothing.                                */
cfd_status cfd_particles_set_mesh(cfd_solver* s, uint32_t num_vertices, const double* vx, const double* vy,
                                  const uint32_t* cell_vertex_offsets /* [N + 1] */,
                                  const uint32_t* cell_vertices /* [cell_vertex_offsets[N]] */,
                                  const uint32_t* face_v1 /* [num_faces] */, const uint32_t* face_v2);
/* A set of `capacity` slots (1..2^24), all EMPTY; 0 frees it.  cfg null: the
 * defaults.  CFD_ERR_INVALID: no mesh, a capacity or hop_cap out of range.    */
cfd_status cfd_particles_enable(cfd_solver* s, uint32_t capacity, const cfd_particle_config* cfg);
/* Overwrites slots [first, first + count): the positions rounded to f32 once,
 * age 0, no contacts, located on the device (ALIVE in a cell, or OUTSIDE).    */
cfd_status cfd_particles_seed(cfd_solver* s, uint32_t first, uint32_t count, const double* x, const double* y);
/* Advances every ALIVE particle by dt; dt <= 0: the dt of the last cfd_step
 * (CFD_ERR_INVALID before any step).  Asynchronous like cfd_step.             */
cfd_status cfd_particles_advance(cfd_solver* s, float dt);
/* Slots [first, first + count); any output may be null.                       */
cfd_status cfd_particles_get(cfd_solver* s, uint32_t first, uint32_t count, float* x, float* y, uint32_t* cell,
                             uint32_t* status, float* age);
cfd_status cfd_particles_stats_get(cfd_solver* s, cfd_particle_stats* out);
/* The last cfd_render frame of the current view with every ALIVE particle in
 * the view stamped as one pixel of rgba_colour (R in the low byte), into
 * rgba[H * W * 4].  All particles store the same value, so the order of the
 * stores does not matter.  The renderer's own frame is not modified.
 * CFD_ERR_INVALID: particles not enabled, no view, no frame of this view yet. */
cfd_status cfd_render_particles(cfd_solver* s, uint32_t rgba_colour, uint8_t* rgba);

/* ------------------------------------------------------------------------ */
/* Time-averaged fields: per-cell running means of u, v, p and of every scalar
 * field, and with second moments the Reynolds stresses <u'u'>, <u'v'>, <v'v'>,
 * <p'p'>, the variances <phi'phi'> and the turbulent fluxes <u'phi'>, <v'phi'>,
 * accumulated on the device one sample per cfd_tstats_accumulate: what a
 * caller could otherwise get only by reading the fields back every step.
 * Opt-in and read-only: a handle that never calls cfd_tstats_enable allocates
 * and launches nothing new, cfd_step launches none of it in any case, and
 * nothing a step reads is written.  One GPU only: handles of
 * cfd_solver_create_dist* and members of a group of more than one rank return
 * CFD_ERR_INVALID.  Beyond the reference, which has no averages.
 * Checkpoints: cfd_state_save / cfd_state_load neither store nor touch the
 * statistics (the file format and its version are unchanged).
 * cfd_tstats_raw_get / cfd_tstats_raw_set and cfd_tstats_info /
 * cfd_tstats_raw_set_totals round-trip the f64 planes and the totals exactly,
 * so a caller who keeps them next to the state file and restores them after
 * cfd_state_load continues the averages bit for bit.
 *
 * Arithmetic of the time statistics.  Everything f64, one rounding per
 * operation, nothing fused.  It is the weighted incremental (West / Welford)
 * update: the first sample is exact, and small fluctuations about a large mean
 * do not cancel.  W is the total weight so far (0 after enable and reset).
 *   host, once per call:   w = (double)weight;  Wn = W + w;  r = w / Wn;
 *                          then W = Wn, samples = samples + 1
 *   per cell i, x_q = (double) of the f32 value, q in {u, v, p, phi_0 ..}:
 *     d_q = x_q - m_q                 (the old mean)
 *     m_q = m_q + r * d_q             (the new mean, stored)
 *     e_q = x_q - m_q                 (the new mean)
 *     M_uu += (w * d_u) * e_u;  M_uv += (w * d_u) * e_v;
 *     M_vv += (w * d_v) * e_v;  M_pp += (w * d_p) * e_p
 *     per field f:  M_ff += (w * d_f) * e_f;  M_uf += (w * d_u) * e_f;
 *                   M_vf += (w * d_v) * e_f
 * u, v, p are the current state (what cfd_get_u / cfd_get_p return), phi_f the
 * field as cfd_get_scalar returns it.  w and r are computed on the host: the
 * device divides nothing.  A mean is its plane; a covariance is its M plane
 * divided by W, on the host in f64 after the read-back.  A NaN in a cell makes
 * that cell's statistics NaN and touches no other cell; no cell's result
 * depends on another's or on any schedule.
 * Planes, in this order (cfd_tstats_raw_get / _set index them): 0 m_u, 1 m_v,
 * 2 m_p; with second moments 3 M_uu, 4 M_uv, 5 M_vv, 6 M_pp; then for every
 * field in turn its mean and M_ff, and with second moments M_uf and M_vf.    */
typedef struct cfd_tstats_config {
  int32_t second_moments;  /* 0: means only; 1: also the M planes of uu, uv, vv, pp                 */
  int32_t scalars;         /* 0: none; 1: every scalar field enabled NOW: its mean and M_ff, and
                              with second_moments M_uf and M_vf                                     */
  int32_t reserved[2];
} cfd_tstats_config;
/* cfd_tstats_get kinds; 7..10 take scalar_index                               */
enum { CFD_TSTATS_U = 0, CFD_TSTATS_V = 1, CFD_TSTATS_P = 2, CFD_TSTATS_UU = 3, CFD_TSTATS_UV = 4, CFD_TSTATS_VV = 5,
       CFD_TSTATS_PP = 6, CFD_TSTATS_PHI = 7, CFD_TSTATS_PHIPHI = 8, CFD_TSTATS_UPHI = 9, CFD_TSTATS_VPHI = 10 };
/* Allocates the planes (8 N bytes each, rounded up to 256) and zeroes them and
 * the totals; cfg null: {1, 1}.  A second call allocates again: the scalar
 * count is fixed here.  CFD_ERR_INVALID: a flag that is neither 0 nor 1.      */
cfd_status cfd_tstats_enable(cfd_solver* s, const cfd_tstats_config* cfg);
cfd_status cfd_tstats_disable(cfd_solver* s); /* frees */
/* W = 0, samples = 0, every plane zeroed                                      */
cfd_status cfd_tstats_reset(cfd_solver* s);
/* One sample of the current state with this weight; weight <= 0: the dt of the
 * last cfd_step (CFD_ERR_INVALID before any).  Asynchronous like cfd_step.
 * CFD_ERR_INVALID, and nothing changes: a NaN or infinite weight; with
 * cfg.scalars, a count of enabled scalar fields other than the one at
 * cfd_tstats_enable (enable the statistics again).                            */
cfd_status cfd_tstats_accumulate(cfd_solver* s, float weight);
/* Any output may be null.                                                     */
cfd_status cfd_tstats_info(cfd_solver* s, uint64_t* samples, double* total_weight, uint32_t* planes);
/* CFD_ERR_INVALID: a kind whose plane is not enabled, a scalar_index outside
 * the fields the statistics hold, no sample yet (W == 0).                     */
cfd_status cfd_tstats_get(cfd_solver* s, int32_t kind, int32_t scalar_index, double* out /* [N] */);
cfd_status cfd_tstats_raw_get(cfd_solver* s, uint32_t plane, double* out /* [N] */);
cfd_status cfd_tstats_raw_set(cfd_solver* s, uint32_t plane, const double* in /* [N] */);
/* total_weight must be finite and >= 0                                        */
cfd_status cfd_tstats_raw_set_totals(cfd_solver* s, uint64_t samples, double total_weight);

/* ------------------------------------------------------------------------ */
/* Monitor history: probe signals and the flow diagnostics recorded on the
 * device, one sample per cfd_monitor_record, read back whenever the caller
 * wants them (the lift history, a wake probe for the shedding frequency).
 * Opt-in, read-only, one GPU only and outside the checkpoint, as the time
 * statistics above.  A ring: sample number k (from 0) goes to slot k %
 * capacity, and cfd_monitor_get addresses the samples still held, oldest
 * first.  A sample holds constants.time and the dt of the last cfd_step (0
 * before any) as they stand on the host at the call, per probe cell u.x, u.y, p
 * and the scalar fields enabled when the monitor was enabled (f32, the values
 * cfd_get_u / cfd_get_p / cfd_get_scalar widen), and with with_diag the device
 * result of the flow-diagnostics pass at that state, decoded on read-back by
 * the code cfd_flow_diagnostics uses: the same bytes it would have returned,
 * the force region of that moment included.                                   */
/* Replaces an earlier monitor.  CFD_ERR_INVALID, and nothing changes: capacity
 * outside 1..2^20, num_probes above 1024, a probe cell >= N.                  */
cfd_status cfd_monitor_enable(cfd_solver* s, uint32_t capacity, uint32_t num_probes,
                              const uint32_t* probe_cells /* [num_probes] */, int32_t with_diag);
cfd_status cfd_monitor_disable(cfd_solver* s); /* frees */
/* Asynchronous: no copy to the host and no synchronisation.  CFD_ERR_INVALID: a
 * count of enabled scalar fields other than the one at cfd_monitor_enable.    */
cfd_status cfd_monitor_record(cfd_solver* s);
/* total: samples ever recorded; held = min(total, capacity).  Either may be null. */
cfd_status cfd_monitor_count(cfd_solver* s, uint64_t* total, uint64_t* held);
/* What cfd_monitor_enable fixed: the capacity, the probes, the scalar fields a
 * probe holds and whether samples carry the diagnostics.  Any may be null.    */
cfd_status cfd_monitor_info(cfd_solver* s, uint32_t* capacity, uint32_t* num_probes, uint32_t* scalar_fields,
                            int32_t* with_diag);
/* Held samples [first, first + count), oldest first.  Any output may be null;
 * probes is [count][num_probes][3 + scalar fields]; diag is zeroed when the
 * monitor was enabled without with_diag.                                      */
cfd_status cfd_monitor_get(cfd_solver* s, uint64_t first, uint64_t count, float* time, float* dt, float* probes,
                           cfd_flow_diag* diag /* [count] */);

/* ------------------------------------------------------------------------ */
/* Wall surface distributions: what cfd_flow_diagnostics, cfd_scalar_wall_flux_get
 * and cfd_wall_motion_get integrate, face by face -- the pressure round a body,
 * the wall shear (its sign change is the separation point), the local heat flux
 * of a heated wall, and their time mean and variance -- evaluated on the device
 * from the current state, so a long run reads back O(sqrt N) f64 values per
 * sample instead of the fields.  Opt-in, read-only, one GPU only and outside
 * the checkpoint, as the time statistics above: a handle that never calls
 * cfd_surface_select allocates and launches nothing new, cfd_step launches none
 * of it in any case, and nothing a step reads is written.  Handles of
 * cfd_solver_create_dist* and members of a group of more than one rank return
 * CFD_ERR_INVALID.
 *
 * A surface is the ordered list of the wall faces whose f64 face centre lies in
 * a closed box: cfd_set_force_region's own rule (one host function serves
 * both), ordered by ascending cell index, then ascending slot in the cell's
 * face list.  It is independent of the force region.
 *
 * Arithmetic of the surface channels.  Everything f64 from the f32 inputs, one
 * rounding per operation, left to right as written, nothing fused.  Face j is
 * slot k of cell i; e = k N + i indexes the face-slot arrays; ad =
 * (double)area[e]; dist = (double)dist_e[e] (the distance the wall diffusion of
 * the momentum equation uses).
 *   0        (double)p[i]
 *   1, 2     (double)p[i] * (double)nx[e] * ad;  (double)p[i] * (double)ny[e] * ad
 *   3, 4     (double)viscosity * rux * ad / dist;  (double)viscosity * ruy * ad / dist
 *            rux = (double)u[i].x, ruy = (double)u[i].y; on a slot the
 *            boundary-velocity selection moves, rux = (double)u[i].x -
 *            (double)ubx and likewise ruy, with ubx = bx * (wall_scale * ramp),
 *            uby = by * (wall_scale * ramp) in f32 ("Arithmetic of boundary
 *            velocities")
 *   5 + 2f   field f's wall-flux term: on a slot of the field's wall selection
 *            (cfd_set_scalar_wall, kind 1 or 2), kind 1: (double)c_k *
 *            ((double)value - (double)phi_f[i]) with c_k = (density * D) *
 *            area[e] / dist_e[e] in f32; kind 2: (double)value * ad; +0 on
 *            every other slot
 *   6 + 2f   (double)phi_f[i]
 * 5 + 2 * (enabled scalar fields) channels.  Channels 1-4 are the force of the
 * fluid on the wall as the assembly discretises it: they are the terms of
 * cfd_flow_diagnostics' force sums, and channel 5 + 2f the terms of
 * cfd_scalar_wall_flux_get's flux.  Adding a cell's terms in slot order from +0
 * and the cells' sums in the canonical order of those calls gives their bits.
 *
 * Statistics: per face and channel x, the weighted incremental (West / Welford)
 * update of "Arithmetic of the time statistics" with the covariance of x with
 * itself:  host, once per call: w = weight; Wn = W + w; r = w / Wn; then W = Wn;
 * device:  d = x - m;  m = m + r * d;  e = x - m;  M2 += (w * d) * e.
 * The evaluation and the update are one kernel launch; the total weight W is
 * kept on the host (the device divides nothing).
 *
 * Configuration changes after cfd_surface_select.  cfd_scalars_enable (any
 * count), cfd_set_scalar_wall and cfd_set_boundary_velocity are accepted; the
 * next cfd_surface_* call re-derives the channel count from the scalar fields
 * enabled then and RESETS the statistics (W = 0, samples = 0, mean and M2
 * zeroed; they stay enabled), because a mean over two channel sets, wall
 * selections or wall conditions means nothing.  The surface's faces stay.
 * Parameter values (viscosity, density, diffusivity, the boundary-velocity
 * scales, the ramp) are read at each call and reset nothing.                  */
typedef struct cfd_surface_info {
  uint32_t faces;
  uint32_t channels;     /* 5 + 2 * the scalar fields enabled now                  */
  uint64_t samples;      /* accumulated since the last reset                       */
  double total_weight;   /* W                                                      */
  int32_t stats_on;
  int32_t reserved;
} cfd_surface_info;
/* Builds and uploads the face table (cell u32, slot u32) and allocates the
 * channel buffers, in device memory of the module's own.  A second call
 * replaces the surface and resets the statistics (they stay enabled).  x1 < x0
 * clears the surface and frees everything; a box without a wall face gives a
 * surface of 0 faces.  n_faces may be null.                                   */
cfd_status cfd_surface_select(cfd_solver* s, double x0, double y0, double x1, double y1, int32_t* n_faces);
/* Per face, any output null or [faces]: its cell and slot, the f64 face centre
 * the selection tested, and the f32 normal (out of the cell, into the wall),
 * area and dist_e the channels are computed from, widened.                    */
cfd_status cfd_surface_geometry_get(cfd_solver* s, uint32_t* cell, uint32_t* slot, double* cx, double* cy, double* nx,
                                    double* ny, double* area, double* dist_e);
/* Like every cfd_surface_* call it is "the next call" of "Configuration changes"
 * above: after such a change this query itself re-derives the channels and
 * resets the statistics, and reports the counts that hold from then on.       */
cfd_status cfd_surface_info_get(cfd_solver* s, cfd_surface_info* out);
/* The channels of the current state: one launch, one copy, out[c * faces + j].
 * CFD_ERR_INVALID: no surface.                                                */
cfd_status cfd_surface_sample(cfd_solver* s, double* out /* [channels * faces] */);
/* on != 0 allocates and zeroes mean and M2; 0 frees them.  No change: no-op.  */
cfd_status cfd_surface_stats_enable(cfd_solver* s, int32_t on);
/* W = 0, samples = 0, mean and M2 zeroed                                      */
cfd_status cfd_surface_stats_reset(cfd_solver* s);
/* One sample of the current state with this weight; weight <= 0: the dt of the
 * last cfd_step (CFD_ERR_INVALID before any).  Asynchronous like cfd_step: one
 * launch, no copy, no synchronisation.  CFD_ERR_INVALID, and nothing changes: a
 * NaN or infinite weight, statistics not enabled.                             */
cfd_status cfd_surface_stats_accumulate(cfd_solver* s, double weight);
/* kind 0: the means; 1: the variances M2 / W, divided on the host in f64 after
 * the read-back (W == 0: the zeros M2 holds).  out[c * faces + j].
 * CFD_ERR_INVALID: statistics not enabled, another kind.                      */
cfd_status cfd_surface_stats_get(cfd_solver* s, int32_t kind, double* out /* [channels * faces] */);

#ifdef __cplusplus
}
#endif
#endif /* CFD2_AMD_H */
