// The byte models: what one step, one V-cycle and one level-0
// smoother sweep move, in the reference's format (algorithmic) and in this
// library's layouts (layout-true).  Nothing here touches the GPU.
#include <algorithm>

#include "solver_impl.hpp"

namespace cfd2 {

// algorithmic bytes of one level-ℓ smoother sweep in the
// reference CSR/f32/u32 format: 4(n+1) + 8 nnz + 12 n.
double Solver::smoother_bytes() const {
  if (levels.empty()) return 0.0;
  const double n = levels[0].dev.n, nnz = (double)levels[0].nnz;
  return 4.0 * (n + 1.0) + 8.0 * nnz + 12.0 * n;
}

// Layout-true bytes of one level-0 sweep of k_amg_smooth: what the kernel
// must move in the AmgLevelDev image -- the u8 row lengths, every ELL slot's
// value and column (16-bit delta or i32) over the padded rows, b, x, the
// smoother diagonal and x_out (4 B each per row; the x gathers at the
// neighbours counted once, as SURVEY §8(d) counts them).  At C2 (w = 4,
// 16-bit deltas) 41 B per row against the reference format's 56.
double Solver::smoother_layout_bytes() const {
  if (levels.empty()) return 0.0;
  const AmgLevelDev& d = levels[0].dev;
  const double st = d.stride, n = d.n;
  return st + std::max(d.w, 1) * st * (4.0 + (d.use16 ? 2.0 : 4.0)) + 16.0 * n;
}

// Layout-true bytes of one V-cycle over the level images: the sum over the
// schedule's ops of what each launch moves (Solver::layout_step_bytes).
// Known undercount, kept: the all-gather, the plain tail and the ten coarsest
// sweeps count nothing.
double Solver::v_cycle_layout_bytes() const {
  auto row_image = [](const AmgLevelDev& d) {  // ELL values + columns over the padded rows
    return std::max(d.w, 1) * (double)d.stride * (4.0 + (d.use16 ? 2.0 : 4.0));
  };
  auto n_of = [&](int i) { return (double)levels[i].dev.n; };
  auto smooth = [&](int i) { return levels[i].dev.stride + row_image(levels[i].dev) + 16 * n_of(i); };
  auto fused_rr = [&](int i) {  // fused residual + restriction
    const double n = n_of(i), nc = n_of(i + 1), st = levels[i].dev.stride;
    return 4 * nc + 4 * n + 2 * st + row_image(levels[i].dev) + 14 * n + 12 * nc;
  };
  // post-smoother reading x + P xc
  auto smooth_prolong = [&](int i) { return smooth(i) + 4 * n_of(i) + 4 * n_of(i + 1); };
  double vc = 0.0;
  for (const VcOp& op : vc_plan) {
    const int i = op.level;
    const double n = n_of(i), st = levels[i].dev.stride;
    switch (op.kind) {
      // pre-smoother (coarse: zero-x, elementwise; not launched when fused into
      // the previous level's restriction, whose 12 nc term counts it)
      case VcKind::PreSmooth: vc += op.flag ? 12 * n : smooth(i); break;
      case VcKind::ResRestrictFused: vc += fused_rr(i); break;
      case VcKind::ResidualRestrict:  // residual, restriction
        vc += (2 * st + row_image(levels[i].dev) + 16 * n) + (16 * n_of(i + 1) + 4 * n + 12 * n_of(i + 1));
        break;
      // k_amg_resrestrict_pair: its second level's b and x stay in LDS
      case VcKind::ResRestrictPair: vc += fused_rr(i) + fused_rr(i + 1) - 8 * n_of(i + 1); break;
      // single-workgroup tail (LDS image in)
      case VcKind::TailBlob: vc += 4.0 * tail_blob_words + 16.0 * tail_vec_floats; break;
      case VcKind::TakePreSmoothed: case VcKind::GatherRhs: case VcKind::Tail: case VcKind::CoarsestSweeps: break;
      case VcKind::Prolong: vc += 12 * n + 4 * n_of(i + 1); break;
      case VcKind::PostSmooth: vc += smooth(i); break;
      case VcKind::PostSmoothProlong: vc += smooth_prolong(i); break;
      // k_amg_prolong_smooth_pair: its coarse level's smoothed x stays in LDS
      case VcKind::ProlongSmoothPair: vc += smooth_prolong(i) + smooth_prolong(i - 1) - 8 * n; break;
    }
  }
  return vc;
}

// Layout-true bytes of one step under the fixed schedule: per kernel, the
// bytes its arrays in THIS library's layouts must move (each element once:
// neighbour gathers counted once, as SURVEY §8(d) counts them), times its
// launches per step: the minimum traffic at kernel level.  It is not a lower
// bound of the HBM traffic: the kernel order is tuned so that some lines come
// from the Infinity Cache, so the PMC step traffic
// (step_counter_traffic) can be below it.
double Solver::layout_step_bytes() const {
  const double Nn = N;
  double S = 0.0, Sint = 0.0;  // used face slots, internal ones
  for (uint32_t i = 0; i < N; ++i) S += topo.nface[i];
  for (uint32_t li = 0; li < N; ++li) Sint += (double)(topo.srow[li + 1] - topo.srow[li]) - 1.0;
  const double ws = topo.ws;
  const int K = cfg.fixed_outer > 0 ? cfg.fixed_outer : std::max(cfg.n_outer_correctors, 10);
  const int M = cfg.fixed_inner > 0 ? std::min(cfg.fixed_inner, m) : m;
  // the VISC forms (viscosity.hpp): mu per cell, 4 B.  The gather mu[other] of every internal slot adds nothing:
  // as with the u / dp gathers here, each cell's value is counted once and the re-reads are assumed to hit cache
  const double visc_bytes = visc.on() ? 4.0 * Nn : 0.0;
  // the PEN forms (penalty.hpp): sigma 4 B, forch 4 B and the target 8 B per cell when set, coalesced, no gather;
  // prepare reads sigma and forch, the assembly the target too
  const double pen_prep = pen.on() ? (4.0 + (pen.has_forch ? 4.0 : 0.0)) * Nn : 0.0;
  const double pen_asmb = pen.on() ? pen_prep + (pen.has_target ? 8.0 : 0.0) * Nn : 0.0;
  const double prep = 40 * S + 60 * Nn + visc_bytes + pen_prep;  // 9 slot arrays + flux out; cell state in, gradients out
  BuoyancyArgs bu;
  const double buoy = scalars.buoyancy_args(bu) ? 4.0 * bu.n * Nn : 0.0;  // the buoyant assembly: one field value per driving field
  const double asmb = 32 * S + 20 * Sint + 78 * Nn + buoy + visc_bytes + pen_asmb;  // 8 slot arrays; 3x3 block + Poisson entry out
  const double spmv = (35 + 16 * ws) * Nn;                 // headers, cval_a + cval_g slots, x, y
  const double predict = (39 + 8 * ws) * Nn;               // headers, cval_g slots, V_j, dinv, temp_p / p_sol out
  const double correct = (34 + 8 * ws) * Nn;               // lg, cval_g slots, p_sol, V_j, dinv, Z_j out
  const double vc = v_cycle_layout_bytes();
  double inner = 0.0;
  for (int j = 0; j < M; ++j) {
    inner += predict + vc + correct + spmv;
    inner += (j + 2) * 12.0 * Nn + (j + 3) * 12.0 * Nn;    // CGS dots, CGS update + norm
  }
  const double residual = spmv + 12 * Nn + 12 * Nn;       // SpMV storing b - A x (b read), norm
  const double solve = 12 * Nn + residual + inner + (M + 2) * 12.0 * Nn + residual;
  return K * (prep + asmb + solve + 36 * Nn);  // prepare: once per Picard iteration (scheme 0)
}

double Solver::algorithmic_step_bytes() const {
  const double Nn = N, Fn = F, S = (double)topo.srow[N] - 0.0;  // nnz_s
  double Sfaces = 0.0;
  for (uint32_t i = 0; i < N; ++i) Sfaces += topo.nface[i];
  const double nnz_s = S;
  // a viscosity per cell: 4 B per cell and 4 B per face (the neighbour's) in prepare and in assemble
  const double visc_bytes = visc.on() ? 4.0 * Nn + 4.0 * Sfaces : 0.0;
  const double pen_prep = pen.on() ? (4.0 + (pen.has_forch ? 4.0 : 0.0)) * Nn : 0.0;  // as in layout_step_bytes
  const double pen_asmb = pen.on() ? pen_prep + (pen.has_target ? 8.0 : 0.0) * Nn : 0.0;
  const double prep = 84 * Nn + 4 * Sfaces + 36 * Fn + visc_bytes + pen_prep;
  BuoyancyArgs bu;
  const double buoy = scalars.buoyancy_args(bu) ? 4.0 * bu.n * Nn : 0.0;  // as in layout_step_bytes
  const double asmb = 68 * Nn + 8 * Sfaces + 36 * Fn + 40 * nnz_s + buoy + visc_bytes + pen_asmb;
  const int K = cfg.fixed_outer > 0 ? cfg.fixed_outer : std::max(cfg.n_outer_correctors, 10);
  const int M = cfg.fixed_inner > 0 ? std::min(cfg.fixed_inner, m) : m;
  // V-cycle bytes
  double vc = 0.0;
  for (size_t li = 0; li < levels.size(); ++li) {
    const double n = levels[li].dev.n, nnz = (double)levels[li].nnz;
    const double bs = 4 * (n + 1) + 8 * nnz + 12 * n;
    if (li + 1 < levels.size()) {
      const double nc = levels[li + 1].dev.n;
      const double br = 4 * (n + 1) + 8 * nnz + 8 * n + 4 * (nc + 1) + 8 * n + 4 * nc;
      const double bp = 4 * (n + 1) + 8 * n + 8 * n + 4 * nc;
      vc += 2 * bs + br + bp + 4 * nc;
    } else {
      vc += 10 * bs;
    }
  }
  double inner = 0.0;
  for (int j = 0; j < M; ++j) {
    inner += 36 * Nn + 72 * nnz_s;                       // SpMV
    inner += (j + 1) * 24.0 * Nn + 36 * Nn;              // CGS
    inner += 12 * Nn + 24 * Nn;                          // norm + scale
    inner += 52 * Nn + 24 * nnz_s + 48 * Nn + 48 * nnz_s + vc;  // preconditioner
  }
  const double solve = inner + M * 36.0 * Nn + 2 * (36 * Nn + 72 * nnz_s) + 36 * Nn + 3 * 12 * Nn;
  return prep + K * (prep + asmb + solve + 36 * Nn);
}

}  // namespace cfd2
