// Test-only entry points: the reference-semantics mode (the reference's own
// reduction orders, racy prepare and in-place smoother under a legal schedule,
// cfd_debug_reference_semantics), the read-backs of cfd_debug_buffer and of
// the AMG levels, and the V-cycle / preconditioner applied outside the solve.
#include <algorithm>

#include "solver_impl.hpp"

namespace cfd2 {

void Solver::set_reference_semantics(int flags) {
  if (flags & ~(1 | 2 | 4 | 8))
    throw std::invalid_argument("reference semantics on the GPU: flags 1 (in-place smoother), 2 (racy prepare), "
                                "4 (reduction order), 8 (restrict clamp) only");
  if (flags && dist()) throw std::invalid_argument("reference semantics: one GPU only");
  if ((flags & 2) && bcv.on())
    throw std::invalid_argument("reference semantics: the racy prepare has no form with prescribed boundary velocities "
                                "(clear them first)");
  if ((flags & (1 | 2)) && visc.on())
    throw std::invalid_argument("reference semantics: the racy prepare and the in-place smoother have no form with a "
                                "viscosity field (clear it first)");
  if ((flags & (1 | 2)) && pen.on())
    throw std::invalid_argument("reference semantics: the racy prepare and the in-place smoother have no form with "
                                "volume penalisation (clear it first)");
  if ((flags & 2) && !d_flux_mirror) {  // each non-owner face slot -> the owner's slot of that face
    const size_t S = (size_t)topo.wf * N;
    size_t nfaces = 0;  // unused slots hold 0xFFFFFFFF: not a face
    for (size_t e = 0; e < S; ++e)
      if (topo.fs_face[e] != 0xFFFFFFFFu) nfaces = std::max(nfaces, (size_t)topo.fs_face[e] + 1);
    std::vector<int64_t> owner_slot(nfaces, -1);
    for (size_t e = 0; e < S; ++e)
      if (topo.fs_face[e] != 0xFFFFFFFFu && (topo.fs_meta[e] & kMetaOwner)) owner_slot[topo.fs_face[e]] = (int64_t)e;
    std::vector<int32_t> mirror(S, -1);
    for (size_t e = 0; e < S; ++e)
      if (topo.fs_face[e] != 0xFFFFFFFFu && topo.fs_other[e] != kNoCell && !(topo.fs_meta[e] & kMetaOwner)) {
        const int64_t o = owner_slot[topo.fs_face[e]];
        if (o < 0) throw std::logic_error("reference semantics: a face without its owner's slot");
        mirror[e] = (int32_t)o;
      }
    d_flux_mirror = arena.upload(mirror, stream);
  }
  if ((flags & 4) && !ref_part) {
    ref_ng = (uint32_t)((3 * (uint64_t)N + 63) / 64);
    ref_part = arena.alloc<float>((size_t)(m1 + 1) * ref_ng + 1);
    ref_norm = arena.alloc<float>((size_t)ref_ng + 1);
  }
  drop_graphs();  // captured iterations hold the other semantics' launches
  ref_red = (flags & 4) != 0;
  ref_inplace = (flags & 1) != 0;
  ref_clamp = (flags & 8) != 0;
  ref_racy = (flags & 2) != 0;
}

// Reference reduction order (test mode): coupled_solver.rs:504-545 literally,
// on the host -- the AoS FluidState view (8 floats per cell: u, v, p, d_p,
// grad_p, grad_component = 0) read at floats 2i, 2i + 1 (the stride bug) and
// serial f64 loops.  tot: evolution, sum u, sum v, sum u^2, sum v^2.
void Solver::evolution_reference(double tot[5]) {
  auto aos = [&](const StateView& v, std::vector<float>& out) {
    std::vector<float> soa(6 * (size_t)N);  // the fields back to back
    size_t o = 0;
    for_each_field(v, [&](float* base, int comps) {
      CFD_HIP(hipMemcpyAsync(soa.data() + o, base, (size_t)N * comps * sizeof(float), hipMemcpyDeviceToHost, stream));
      o += (size_t)N * comps;
    });
    sync();
    out.assign(8 * (size_t)N, 0.0f);
    const float* s = soa.data();
    int k = 0;  // a record: u, v, p, d_p, grad_p x, y
    for_each_field(v, [&](float*, int comps) {
      for (size_t c = 0; c < N; ++c, s += comps) std::copy_n(s, comps, out.data() + 8 * c + k);
      k += comps;
    });
  };
  std::vector<float> cur, old;
  aos(S(), cur);
  double e = 0.0, a = 0.0, b = 0.0, aa = 0.0, bb = 0.0;
  if (have_prev) {
    aos(prev, old);
    for (size_t k = 0; k < cur.size(); ++k) {
      const float d = cur[k] - old[k];
      e += (double)(d * d);
    }
  }
  for (size_t c = 0; c < N; ++c) {
    const double u = (double)cur[2 * c], v = (double)cur[2 * c + 1];
    a += u;
    b += v;
    aa += u * u;
    bb += v * v;
  }
  tot[0] = e;
  tot[1] = a;
  tot[2] = b;
  tot[3] = aa;
  tot[4] = bb;
}

void Solver::debug_prepare_assemble(bool asmb) {
  CFD_HIP(hipSetDevice(device));
  constants.component = 0;
  prepare();
  if (asmb) assemble();
  sync();
}

// One level as plain CSR from the arrays the V-cycle kernels read: the
// off-diagonal slots (level_csr: u8 or, on a wide level, u16 lengths; 16-bit
// deltas or 32-bit columns), the diagonal put back at its rank with the value
// dv, then dv / de and the transfer operators.  Sizes first; arrays when the
// caller passes them.
void Solver::debug_amg_level(int li, cfd_amg_level* io) {
  if (dist()) throw std::invalid_argument("AMG level read-back: one GPU only");
  if (!amg_built) throw std::invalid_argument("AMG level read-back: no hierarchy built yet");
  if (li < 0 || li >= (int)levels.size()) throw std::invalid_argument("no such AMG level");
  CFD_HIP(hipSetDevice(device));
  const AmgGpuLevel& G = levels[li];
  const AmgLevelDev& d = G.dev;
  const uint32_t n = d.n, nc = d.nc;
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) CFD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
  };
  std::vector<uint32_t> r_row((size_t)(nc ? nc + 1 : 0));
  d2h(r_row.data(), d.r_row, r_row.size() * 4);
  sync();
  const size_t r_nnz = nc ? r_row[nc] : 0;
  const bool fill = io->row || io->col || io->val || io->dv || io->de || io->agg || io->r_row || io->r_col ||
                    io->m4 || io->m4_more;
  if (fill && (io->n != n || io->nc != nc || io->nnz != G.nnz || io->r_nnz != r_nnz))
    throw std::invalid_argument("AMG level read-back: the sizes are not those of the first call");
  io->n = n;
  io->nc = nc;
  io->nnz = G.nnz;
  io->r_nnz = r_nnz;
  io->wide = d.len16 ? 1 : 0;  // what the kernels read
  io->use16 = d.use16;
  if (!fill) return;
  // ---- the matrix ----
  std::vector<uint8_t> dr8(d.drank16 ? 0 : n);
  std::vector<uint16_t> dr(n);
  std::vector<float> dv(n), de(n);
  if (d.drank16) d2h(dr.data(), d.drank16, (size_t)n * 2);
  else d2h(dr8.data(), d.drank, n);
  d2h(dv.data(), d.dv, (size_t)n * 4);
  d2h(de.data(), d.de, (size_t)n * 4);
  std::vector<uint32_t> orow, ocol;
  std::vector<float> oval;
  if (!level_csr(d, orow, ocol, &oval)) throw std::logic_error("AMG level read-back: a column outside the level");
  if (!d.drank16) std::copy(dr8.begin(), dr8.end(), dr.begin());
  if ((uint64_t)orow[n] + n != G.nnz)
    throw std::logic_error("AMG level read-back: the image's row lengths do not add up to the level's nnz");
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t o0 = orow[i], len = orow[i + 1] - o0;
    if (dr[i] > len) throw std::logic_error("AMG level read-back: a diagonal rank past its row");
    const size_t k0 = (size_t)o0 + i;  // i diagonals precede row i
    if (io->row) io->row[i] = (uint32_t)k0;
    for (uint32_t r = 0; r <= len; ++r) {
      const bool diag = r == dr[i];
      const uint32_t src = o0 + (r > dr[i] ? r - 1 : r);
      if (io->col) io->col[k0 + r] = diag ? i : ocol[src];
      if (io->val) io->val[k0 + r] = diag ? dv[i] : oval[src];
    }
  }
  if (io->row) io->row[n] = (uint32_t)G.nnz;
  if (io->dv) std::copy(dv.begin(), dv.end(), io->dv);
  if (io->de) std::copy(de.begin(), de.end(), io->de);
  if (!nc) return;
  // ---- P, R and the 4-member image of R ----
  std::vector<int32_t> m4(4 * (size_t)nc);
  if (io->agg) d2h(io->agg, d.agg, (size_t)n * 4);
  if (io->r_col) d2h(io->r_col, d.r_col, r_nnz * 4);
  d2h(m4.data(), d.r_m4, m4.size() * 4);
  sync();
  if (io->r_row) std::copy(r_row.begin(), r_row.end(), io->r_row);
  for (uint32_t I = 0; I < nc; ++I) {
    const int32_t w = m4[4 * (size_t)I + 3];  // < -1: more than four members, member 3 = -2 - w
    for (int q = 0; q < 4 && io->m4; ++q) io->m4[4 * (size_t)I + q] = (q == 3 && w < -1) ? -2 - w : m4[4 * (size_t)I + q];
    if (io->m4_more) io->m4_more[I] = w < -1 ? 1 : 0;
  }
}

// apply_precond's cycle on caller-given vectors: eager launches on the solver's
// stream (no graph is being captured between steps), level 0 bound to
// (p_sol, temp_p) as every cycle binds it.  Both vectors are rewritten by the
// next Schur prediction before anything reads them.
void Solver::debug_amg_vcycle(const float* x0, const float* b, float* out, size_t n) {
  if (dist()) throw std::invalid_argument("AMG V-cycle call: one GPU only");
  if (!amg_built || !fgmres_ready) throw std::invalid_argument("AMG V-cycle call: no hierarchy built yet");
  if (n != N || !x0 || !b || !out) throw std::invalid_argument("AMG V-cycle call: vectors of num_cells floats");
  if (capturing) throw std::logic_error("AMG V-cycle call inside a graph capture");
  CFD_HIP(hipSetDevice(device));
  CFD_HIP(hipMemcpyAsync(p_sol, x0, (size_t)N * 4, hipMemcpyHostToDevice, stream));
  CFD_HIP(hipMemcpyAsync(temp_p, b, (size_t)N * 4, hipMemcpyHostToDevice, stream));
  v_cycle();
  check_launch("AMG V-cycle (debug call)");
  CFD_HIP(hipMemcpyAsync(out, p_sol, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
  sync();
}

// precondition(0, Z_0) on a caller-given V_0 (binv[0] = 1: V_0 is read as it
// is).  Basis slot 0, binv[0], Z slot 0 and the pressure scratch are written
// by every solve's start and first iteration before they are read.
void Solver::debug_apply_precond(const float* v, float* z, size_t n3) {
  if (dist()) throw std::invalid_argument("preconditioner call: one GPU only");
  if (!fgmres_ready) throw std::invalid_argument("preconditioner call: no step solved yet");
  if (constants.precond_type == 1 && !amg_built)
    throw std::invalid_argument("preconditioner call: no hierarchy built yet");
  if (n3 != 3 * (size_t)N || !v || !z) throw std::invalid_argument("preconditioner call: vectors of 3 num_cells floats");
  if (capturing) throw std::logic_error("preconditioner call inside a graph capture");
  CFD_HIP(hipSetDevice(device));
  const float one = 1.0f;
  CFD_HIP(hipMemcpyAsync(basis, v, n3 * 4, hipMemcpyHostToDevice, stream));
  CFD_HIP(hipMemcpyAsync(binv, &one, 4, hipMemcpyHostToDevice, stream));
  precondition(0, zvec);
  check_launch("preconditioner (debug call)");
  CFD_HIP(hipMemcpyAsync(z, zvec, n3 * 4, hipMemcpyDeviceToHost, stream));
  sync();
}

size_t Solver::debug_len(int id) const {
  const size_t n = N;
  switch (id) {
    case 0: return F;
    case 1: case 2: case 10: case 11: case 12: return 2 * n;
    case 3: case 4: return 3 * n;
    case 5: case 6: case 7: return n;
    case 8: return topo.scol.size();
    case 9: return 9 * topo.scol.size();
    default: return 0;
  }
}

void Solver::debug_buffer(int id, float* out) {
  CFD_HIP(hipSetDevice(device));
  if (dist() && (id == 0 || id == 8 || id == 9))
    throw std::invalid_argument("debug buffers 0/8/9 use the global face/CSR layout (single GPU only)");
  const size_t n = N;
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    CFD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    sync();
  };
  switch (id) {
    case 0: {  // fluxes[face] as written by the owner (prepare_coupled.wgsl:197-200)
      std::vector<float> fsv((size_t)topo.wf * n);
      d2h(fsv.data(), flux_s, fsv.size() * 4);
      std::fill(out, out + F, 0.0f);
      for (size_t e = 0; e < fsv.size(); ++e) {
        const uint32_t i = (uint32_t)(e % n), k = (uint32_t)(e / n);
        if (k < topo.nface[i] && (topo.fs_meta[e] & kMetaOwner)) out[topo.fs_face[e]] = fsv[e];
      }
      break;
    }
    case 1: d2h(out, grad_u, 2 * n * 4); break;
    case 2: d2h(out, grad_v, 2 * n * 4); break;
    case 3: d2h(out, rhs, 3 * n * 4); break;
    case 4: d2h(out, x, 3 * n * 4); break;
    case 5: case 6: d2h(out, dinv_uv, n * 4); break;
    case 7: d2h(out, dinv_p, n * 4); break;
    case 8: {
      const size_t ld = topo.ld;
      std::vector<float> ell((size_t)topo.ws * ld);
      d2h(ell.data(), sval, ell.size() * 4);
      for (uint32_t i = 0; i < N; ++i)
        for (uint32_t k = topo.srow[i]; k < topo.srow[i + 1]; ++k) out[k] = ell[(size_t)(k - topo.srow[i]) * ld + i];
      break;
    }
    case 9: {  // expand compressed blocks to the reference CSR (init/linear_solver/mod.rs:180-216)
      const size_t ld = topo.ld;
      std::vector<float2> ca((size_t)topo.ws * ld), cg((size_t)topo.ws * ld);
      std::vector<float2> d2(n);
      d2h(ca.data(), cval_a, ca.size() * sizeof(float2));
      d2h(cg.data(), cval_g, cg.size() * sizeof(float2));
      d2h(d2.data(), cdiag2, n * sizeof(float2));
      for (uint32_t i = 0; i < N; ++i) {
        const uint32_t so = topo.srow[i], nb = topo.srow[i + 1] - so;
        const uint32_t r0 = 9 * so, r1 = r0 + 3 * nb, r2 = r0 + 6 * nb;
        for (uint32_t r = 0; r < nb; ++r) {
          const size_t e = (size_t)topo.tslot[so + r] * ld + i;  // aligned slot of CSR entry r
          const float2 a = ca[e], gg = cg[e];
          const bool diag = (r == topo.ell_drank[i]);
          out[r0 + 3 * r + 0] = a.x;
          out[r0 + 3 * r + 1] = 0.0f;
          out[r0 + 3 * r + 2] = gg.x;
          out[r1 + 3 * r + 0] = 0.0f;
          out[r1 + 3 * r + 1] = a.x;
          out[r1 + 3 * r + 2] = gg.y;
          out[r2 + 3 * r + 0] = diag ? d2[i].x : gg.x;
          out[r2 + 3 * r + 1] = diag ? d2[i].y : gg.y;
          out[r2 + 3 * r + 2] = a.y;
        }
      }
      break;
    }
    case 10: d2h(out, S().gp, 2 * n * 4); break;
    case 11: d2h(out, ring[i_old].u, 2 * n * 4); break;
    case 12: d2h(out, ring[i_old_old].u, 2 * n * 4); break;
    default: throw std::invalid_argument("unknown debug buffer id");
  }
}

}  // namespace cfd2
