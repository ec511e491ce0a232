// FGMRES(50) with the Schur preconditioner (coupled_solver_fgmres.rs:1728-2448
// solve_coupled_fgmres, :212-1280 its lazily created resources).  Host round
// trips are the ones the reference control flow needs (blocking norms at solve
// start / restart, lagged residual reads), and none under the fixed benchmark
// schedule except the two early-exit norms.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "solver_impl.hpp"

namespace cfd2 {

// device scalars dsc[0..15]: rhs_norm, resid, inv_resid, wnorm, inv_w, resid_est
constexpr int kHOff = 16;

void Solver::ensure_fgmres() {  // coupled_solver_fgmres.rs:212-1280 (lazy)
  if (fgmres_ready) return;
  // Krylov vectors in the per-cell layout (ghost space: V_j and Z_j are read at
  // neighbours by the Schur prediction and the SpMV); 256-byte aligned slots
  stride = (3 * vlen + 63) & ~(size_t)63;
  float* braw = arena.alloc<float>((size_t)m1 * stride + 64);
  float* zraw = arena.alloc<float>((size_t)m * stride + 64);
  CFD_HIP(hipMemsetAsync(braw, 0, ((size_t)m1 * stride + 64) * sizeof(float), stream));
  CFD_HIP(hipMemsetAsync(zraw, 0, ((size_t)m * stride + 64) * sizeof(float), stream));
  basis = braw + 3 * (size_t)shift;
  zvec = zraw + 3 * (size_t)shift;
  w = valloc<float>(3);
  // pressure vectors: padded to a multiple of 64 owned rows (the AMG level-0
  // kernels process 4 rows per thread with 16-byte loads), plus ghosts
  temp = valloc<float>(1);
  temp_p = valloc<float>(1);
  p_sol = valloc<float>(1);
  partial = arena.alloc<float>((size_t)m1 * pstride);
  partial_n = arena.alloc<float>(pstride);
  const size_t nsc = kHOff + (size_t)m1 * m + 2 * (size_t)m + m1 + m + m + m1;
  dsc = arena.alloc<float>(nsc);
  CFD_HIP(hipMemsetAsync(dsc, 0, nsc * sizeof(float), stream));
  H = dsc + kHOff;
  givens = H + (size_t)m1 * m;
  g = givens + 2 * m;
  y = g + m1;
  resid_hist = y + m;
  binv = resid_hist + m;
  inner.create(1, h_pin + kPinInner);  // the two pinned residual slots (Solver::solve)
  fgmres_ready = true;
}

// FGMRES Preconditioner Step (coupled_solver_fgmres.rs:1911-1994)
void Solver::precondition(int j, float* z) {
  const CoupledMatrix A = cmat();
  const bool jacobi = constants.precond_type != 1;
  float* v = basis + (size_t)j * stride;  // V_j = binv[j] * W_j
  // the prediction reads neighbours' r_u, r_v
  const CommScope cs(this, kCommKrylovHalo);
  overlapped(cell_plan, {{v, 3}}, N, [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
    const CoupledMatrix Ar = with_rows(A, a, b, a2, b2);
    launch_precond_predict(Ar, v, binv, j, dinv_uv, dinv_p, temp_p, p_sol, jacobi ? temp : nullptr, stream, nt(4));
  });
  bool in_sol = true;
  if (!jacobi) {
    v_cycle();
  } else {
    // p_iters of coupled_solver_fgmres.rs:1949-1976 (global cell count)
    const size_t raw = 20u + (size_t)std::sqrt((float)NG) / 2u;
    const size_t p_iters = std::min<size_t>(raw, 200) == 0 ? 0 : std::min<size_t>(raw, 200) - 1;
    // small meshes: every sweep in one single-workgroup launch (same bits)
    if (!dist() && small_forms &&
        launch_relax_pressure_fused(N, topo.ld, (uint32_t)topo.ws, d_scol, d_slen, sval, dinv_p, temp_p, p_sol, temp,
                                    (uint32_t)p_iters, stream)) {
      if (p_iters & 1) in_sol = false;
    } else {
      AmgLevelDev rv{};  // the scalar ELL image (diagonal in the slots) as a row-kernel level
      rv.n = N;
      rv.r1 = N;
      rv.stride = topo.ld;
      rv.w = topo.ws;
      rv.use16 = topo.use16 ? 1 : 0;
      rv.full = 1;
      rv.val = sval;
      rv.col16 = d_scol16;
      rv.col32 = d_scol;
      rv.len = d_slen8;
      for (size_t it = 0; it < p_iters; ++it) {
        float* src = in_sol ? p_sol : temp;
        float* dst = in_sol ? temp : p_sol;
        if (dist()) halo(cell_plan, {{src, 1}});
        launch_relax_pressure4(rv, d_sdrank8, dinv_p, temp_p, src, dst, stream);
        in_sol = !in_sol;
      }
    }
  }
  float* ps = in_sol ? p_sol : temp;
  // the velocity correction reads neighbours' p_sol
  overlapped(cell_plan, {{ps, 1}}, N, [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
    const CoupledMatrix Ar = with_rows(A, a, b, a2, b2);
    launch_precond_correct(Ar, v, binv, j, ps, dinv_uv, z, stream);
  });
}

void Solver::norm_launch(const float* v, int mode, int slot) {
  if (ref_red) {  // gpu_norm: norm_sq_partial + reduce_final (coupled_solver_fgmres.rs:1444-1588)
    launch_ref_norm_partials(v, 3 * N, ref_norm, stream);
    launch_reduce_final(ref_src(ref_norm, 1), mode, dsc + slot, binv, mode == 2 ? g : nullptr, m1, d_pin + slot,
                        stream);
    return;
  }
  launch_dot_partial(v, v, N, red.U, partial_n, stream);
  // the norm also lands in h_pin[slot] (mapped pinned memory): a blocking read needs no copy
  launch_reduce_final(combine(partial_n, 1), mode, dsc + slot, binv, mode == 2 ? g : nullptr, m1, d_pin + slot,
                      stream);
}

// compute_residual_into (coupled_solver_fgmres.rs:1637-1667): V0 = b - A x, ||V0||
// V0 is stored unnormalised: binv[0] = 1/||r|| (the reference's scale_in_place),
// g = [||r||, 0, ...] (coupled_solver_fgmres.rs:1880-1890, 2380-2392).
float Solver::residual_into_v0_blocking() {
  residual_into_v0_launch();
  sync();
  return h_pin[1];
}

void Solver::residual_into_v0_launch() {
  // g = [||r||, 0, ...]: the zero fill is part of the norm's finishing kernel
  const CommScope cs(this, kCommKrylovHalo);
  overlapped(cell_plan, {{x, 3}}, N, [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
    // V0 = 1 * b + -1 * (A x) as the SpMV stores it
    launch_spmv(with_rows(cmat(), a, b, a2, b2), x, basis, stream, rhs, nt(8));
  });
  norm_launch(basis, 2, 1);
}

// FGMRES iteration j (coupled_solver_fgmres.rs:1911-2283): Z_j = M^-1 V_j,
// w = A Z_j, CGS against V_0..V_j, ||w||, Hessenberg column + Givens.  The
// residual estimate also lands in pinned host memory at `pin` (natural
// schedule) -- no host reads in between, so the sequence is graph-capturable.
void Solver::iteration(int j, float* pin) {
  float* zj = zvec + (size_t)j * stride;
  precondition(j, zj);
  const CommScope cs(this, kCommKrylovHalo);
  overlapped(cell_plan, {{zj, 3}}, N, [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
    launch_spmv(with_rows(cmat(), a, b, a2, b2), zj, w, stream, nullptr, nt(8));
  });
  const bool lat = small_forms && cgs_latency_form(N);
  if (ref_red) {  // calc_dots_cgs / reduce_dots_cgs / update_w_cgs, then norm_sq_partial + finish
    launch_ref_cgs_dots(w, basis, binv, stride, j, 3 * N, ref_part, ref_ng, stream);
    launch_cgs_reduce(ref_src(ref_part, 2), j, H, m1, stream);
    launch_cgs_update_norm(w, basis, binv, stride, j, H, m1, N, red.U, partial_n, stream, cgs_keep_bytes > 0, true,
                           nullptr, lat);
    launch_ref_norm_partials(basis + (size_t)(j + 1) * stride, 3 * N, ref_norm, stream);
    launch_norm_givens(ref_src(ref_norm, 1), j, H, m1, givens, g, binv, resid_hist, pin, stream);
    check_launch("FGMRES iteration (reference reduction order)");
    return;
  }
  launch_cgs_dots(w, basis, binv, stride, j, N, red.U, partial, pstride, stream, cgs_keep_bytes, lat);
  const RedSrc dots = combine(partial, j + 1);
  const bool fuse_reduce = small_forms && cgs_reduce_fusable(dots);
  if (!fuse_reduce) launch_cgs_reduce(dots, j, H, m1, stream);
  // the whole restart basis and w within the kept bytes (small meshes): the
  // dots pass already reads every block with the default policy
  // (launch_cgs_dots), and the update reads / writes the basis with it too,
  // from the caches.  C0 21.2 -> 12.4 us per launch, -1.3 to -1.6 ms/step;
  // on C1's first iterations alone (the j + 2 vectors fitting) it lost
  // ≈ 0.1-0.2 ms/step, hence the whole-basis test (profiles/r05/ab_log.md).
  const bool basis_kept = (size_t)(m1 + 1) * 12u * N <= cgs_keep_bytes;
  launch_cgs_update_norm(w, basis, binv, stride, j, H, m1, N, red.U, partial_n, stream, cgs_keep_bytes > 0,
                         !basis_kept, fuse_reduce ? &dots : nullptr, lat);
  launch_norm_givens(combine(partial_n, 1), j, H, m1, givens, g, binv, resid_hist, pin, stream);
  check_launch("FGMRES iteration (Schur preconditioner, V-cycle, SpMV, CGS)");
}

void Solver::drop_graphs() {
  if (graphs.empty()) return;
  sync();
  for (IterGraph& G : graphs) {
    graph_harvest(G, false);
    if (G.exec) CFD_HIP(hipGraphExecDestroy(G.exec));
    for (auto e : G.ev) CFD_HIP(hipEventDestroy(e));
  }
  graphs.clear();
}

void Solver::graph_harvest(IterGraph& G, bool discard) {
  if (!G.pending) return;
  G.pending = false;
  if (G.ev.empty() || discard) return;
  CFD_HIP(hipEventSynchronize(G.ev.back()));
  for (size_t k = 0; k + 1 < G.ev.size(); k += 2) {
    float ms = 0.0f;
    CFD_HIP(hipEventElapsedTime(&ms, G.ev[k], G.ev[k + 1]));
    prof_ms += ms;
    prof_launches++;
  }
}

void Solver::graph_harvest_all(bool discard) {
  for (IterGraph& G : graphs) graph_harvest(G, discard);
}

void Solver::run_iteration(int j, float* pin, int variant) {
  const bool use = graph_on && !dist() && !check_sync && !comm_prof;
  if (!use) {
    iteration(j, pin);
    return;
  }
  if (graph_precond != (int)constants.precond_type) {
    drop_graphs();
    graph_precond = (int)constants.precond_type;
  }
  if (graphs.empty()) graphs.resize(3 * (size_t)m);
  IterGraph& G = graphs[3 * (size_t)j + variant];
  if (G.exec && G.prof != prof) {  // timing switched on / off: capture again
    sync();
    graph_harvest(G, false);
    CFD_HIP(hipGraphExecDestroy(G.exec));
    for (auto e : G.ev) CFD_HIP(hipEventDestroy(e));
    G = IterGraph{};
  }
  if (!G.exec) {
    hipGraph_t gr = nullptr;
    CFD_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    capturing = &G;
    // a failed capture or instantiation leaves no timing pairs behind: they
    // were never recorded, and a later capture must not append after them
    auto reset_graph = [&] {
      for (auto ev : G.ev) (void)hipEventDestroy(ev);
      G = IterGraph{};
    };
    try {
      iteration(j, pin);
    } catch (...) {
      capturing = nullptr;
      (void)hipStreamEndCapture(stream, &gr);
      if (gr) (void)hipGraphDestroy(gr);
      reset_graph();
      throw;
    }
    capturing = nullptr;
    const hipError_t ec = hipStreamEndCapture(stream, &gr);
    const hipError_t e = ec == hipSuccess ? hipGraphInstantiate(&G.exec, gr, nullptr, nullptr, 0) : ec;
    if (gr) (void)hipGraphDestroy(gr);
    if (e != hipSuccess) {
      G.exec = nullptr;
      reset_graph();
      CFD_HIP(e);
    }
    G.prof = prof;
    graph_captures++;
  }
  graph_harvest(G, false);  // the previous replay's smoother times (complete by now: a solve start synchronised)
  CFD_HIP(hipGraphLaunch(G.exec, stream));
  G.pending = true;
  graph_replays++;
}

cfd_linear_stats Solver::solve() {  // coupled_solver_fgmres.rs:1728-2448
  const Range range("fgmres solve");
  // LinearSolverStats.time = start_time.elapsed() on every exit
  // (coupled_solver_fgmres.rs:1729,1840,1867,2446): host wall time of the solve
  const auto t_start = std::chrono::steady_clock::now();
  auto elapsed = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
  cfd_linear_stats st{};
  const size_t n = 3 * (size_t)N;
  const float tol = cfg.fgmres_rtol, abstol = cfg.fgmres_atol;
  const bool fixed = cfg.fixed_inner > 0;
  const int lag = cfg.convergence_lag;
  ensure_fgmres();
  if (constants.precond_type == 1) ensure_amg();
  // ||b|| and the initial residual V0 = b - A x, ||V0|| in one submission and
  // one readback: the reference reads ||b|| first and skips the residual on
  // its early exit; computing it anyway only writes solver scratch (V0,
  // binv[0], g) that the next solve rewrites, so the results are unchanged
  norm_launch(rhs, 1, 0);  // -> h_pin[0]
  residual_into_v0_launch();  // -> h_pin[1]
  sync();
  const float rhs_norm = h_pin[0];
  if (rhs_norm < abstol || !std::isfinite(rhs_norm)) {
    st.residual = rhs_norm;
    st.converged = rhs_norm < abstol;
    st.diverged = !std::isfinite(rhs_norm);
    st.time_s = elapsed();
    return st;
  }
  float residual_norm = h_pin[1];
  const float target = std::fmax(tol * rhs_norm, abstol);
  if (residual_norm < target) {
    log("FGMRES: Initial guess already converged (||r|| = %s < %s)\n", e2(residual_norm).c_str(), e2(target).c_str());
    st.residual = residual_norm;
    st.converged = 1;
    st.time_s = elapsed();
    return st;
  }
  log("FGMRES: Initial residual = %s\n", e2(residual_norm).c_str());
  uint32_t total = 0;
  float final_resid = residual_norm;
  bool converged = false;
  int stagnation = 0;
  float prev_resid = residual_norm;
  const int inner_max = fixed ? std::min(cfg.fixed_inner, m) : m;
  const int outer_max = fixed ? 1 : cfg.max_outer_restarts;
  for (int outer = 0; outer < outer_max; ++outer) {
    int basis_size = 0;
    for (int j = 0; j < inner_max; ++j) {
      const Range it_range("fgmres iteration");
      basis_size = j + 1;
      ++total;
      // the residual estimate goes to one of two pinned slots, never the slot
      // of a lagged read still pending (which may carry over from the previous
      // iteration, restart or solve: the reader is never reset).  The slot the
      // kernel writes, the graph variant that captured that write and the slot
      // submitted below all come from this one call.
      const int wslot = inner.write_slot();
      run_iteration(j, fixed ? nullptr : d_pin + kPinInner + wslot, fixed ? 0 : 1 + wslot);
      if (fixed) continue;
      // async residual read with the lag model (async_buffer.rs):
      // k_norm_givens wrote resid_hist[j] into the slot; the reader's event orders the read
      inner.submit(wslot, stream, lag);
      const float check = inner.last();
      if (inner.have() && (total % 10 == 0 || check < tol * rhs_norm))
        log("FGMRES iter %u: residual = %s (target %s)\n", total, e2(check).c_str(), e2(tol * rhs_norm).c_str());
      if (inner.have() && check < tol * rhs_norm) {
        converged = true;
        break;
      }
    }
    launch_solve_triangular(H, g, y, basis_size, m1, stream);
    launch_update_x(x, zvec, stride, y, basis_size, n, stream, small_forms);  // 0: the streaming form
    check_launch("FGMRES solution update");
    if (converged) {  // async_reader.flush()
      inner.flush();
      final_resid = inner.last();
      log("FGMRES restart %d: estimated residual = %s\n", outer + 1, e2(final_resid).c_str());
      break;
    }
    residual_norm = residual_into_v0_blocking();
    final_resid = residual_norm;
    if (fixed) {
      converged = residual_norm < tol * rhs_norm;
      break;
    }
    if (residual_norm < tol * rhs_norm) {
      converged = true;
      log("FGMRES restart %d: true residual = %s (converged)\n", outer + 1, e2(residual_norm).c_str());
      break;
    }
    if (residual_norm <= 0.0f) {
      log("FGMRES: residual vanished at restart %d\n", outer + 1);
      converged = true;
      break;
    }
    const float improvement = (prev_resid - residual_norm) / prev_resid;
    if (improvement < 1e-3f) {
      if (++stagnation >= 3) {
        log("FGMRES: Stagnation detected at restart %d (residual %s)\n", outer + 1, e2(residual_norm).c_str());
        converged = true;
        break;
      }
    } else {
      stagnation = 0;
    }
    prev_resid = residual_norm;
    log("FGMRES restart %d: residual = %s (target %s)\n", outer + 1, e2(residual_norm).c_str(),
        e2(tol * rhs_norm).c_str());
  }
  log("FGMRES finished: %u iterations, residual = %s, converged = %s\n", total, e2(final_resid).c_str(),
      tf(converged));
  st.iterations = total;
  st.residual = final_resid;
  st.converged = converged;
  st.diverged = std::isnan(final_resid);
  st.time_s = elapsed();
  return st;
}

}  // namespace cfd2
