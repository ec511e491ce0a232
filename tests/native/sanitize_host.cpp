// Host sanitizer driver for the product's host-side setup code (no GPU):
// slab topology + halo plans for 1-4 ranks, and the host AMG hierarchy
// (greedy aggregation, R = P^T, Galerkin products) with partition-aware
// aggregation, and the V-cycle schedules planned over it, on a cut-cell, a
// Voronoi and a Delaunay mesh.  Built with ASan + UBSan by
// tests/test_sanitize.py; consistency checks on the way.
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../cfd-demo2_amd/csrc/host/solver_impl.hpp"
#include "../../cfd-demo2_amd/csrc/mesh/mesh.hpp"

namespace {

cfd_mesh_view view_of(const cfd2::Mesh& x) {
  cfd_mesh_view v{};
  v.num_cells = x.num_cells();
  v.num_faces = x.num_faces();
  v.face_owner = x.face_owner.data();
  v.face_neighbor = x.face_neighbor.data();
  v.face_boundary = x.face_boundary.data();
  v.face_area = x.face_area.data();
  v.face_nx = x.face_nx.data();
  v.face_ny = x.face_ny.data();
  v.face_cx = x.face_cx.data();
  v.face_cy = x.face_cy.data();
  v.cell_cx = x.cell_cx.data();
  v.cell_cy = x.cell_cy.data();
  v.cell_vol = x.cell_vol.data();
  v.cell_face_offsets = x.cell_face_offsets.data();
  v.cell_faces = x.cell_faces.data();
  return v;
}

void check(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(what);
}

// Invariants of a V-cycle schedule (plan_v_cycle) whatever the flags: sweeps
// per level, every rhs produced once before its first reader, pairs only where
// flagged and disjoint, levels from the tail on in one op.
void check_schedule(const std::vector<cfd2::VcLevel>& lv, int tail_first, bool lds) {
  using K = cfd2::VcKind;
  const int L = (int)lv.size(), down = cfd2::v_cycle_down(tail_first, L);
  const std::vector<cfd2::VcOp> ops = cfd2::plan_v_cycle(lv, tail_first, lds);
  std::vector<int> sweeps(L, 0), rhs(L, 0), in_pair_down(L, 0), in_pair_up(L, 0);
  rhs[0] = 1;  // level 0's rhs is bound by the caller
  int bottom = 0;
  auto reads = [&](int l) { check(l >= 0 && l < L && rhs[l] == 1, "op reads an rhs not produced exactly once"); };
  for (const cfd2::VcOp& op : ops) {
    const int i = op.level;
    check(i >= 0 && i < L, "op level");
    const bool tail_op = op.kind == K::TailBlob || op.kind == K::Tail || op.kind == K::CoarsestSweeps;
    check(tail_op || i < down || (op.kind == K::GatherRhs && i == down),
          "a level from the tail on outside the tail op");
    switch (op.kind) {
      case K::PreSmooth:
        reads(i);
        check(op.flag == (i > 0), "zero-x pre-smoother exactly on the coarse levels");
        sweeps[i]++;
        break;
      case K::TakePreSmoothed:
        reads(i);
        check(sweeps[i] == 1, "takes a pre-smoothed buffer nothing produced");
        break;
      case K::ResRestrictFused:
      case K::ResidualRestrict:
        reads(i);
        check((op.kind == K::ResRestrictFused) == (lv[i].fused_rr && !lv[i].dist), "fused restriction where flagged");
        rhs[i + 1]++;
        if (op.flag) sweeps[i + 1]++;
        check(!op.flag || i + 1 < down, "fused pre-smoother of a level the down leg does not run");
        break;
      case K::ResRestrictPair:
        reads(i);
        check(lv[i].down_pair && i + 2 <= down, "down-leg pair without its flag or past the leg");
        check(!in_pair_down[i] && !in_pair_down[i + 1], "down-leg pairs overlap");
        in_pair_down[i] = in_pair_down[i + 1] = 1;
        rhs[i + 1]++;
        rhs[i + 2]++;
        sweeps[i + 1]++;
        if (op.flag) sweeps[i + 2]++;
        check(!op.flag || i + 2 < down, "fused pre-smoother of a level the down leg does not run");
        break;
      case K::GatherRhs:
        check(i >= 1 && lv[i - 1].dist && !lv[i].dist && rhs[i] == 1, "gather into the first replicated level");
        break;
      case K::TailBlob:
      case K::Tail:
        reads(i);
        check(i == tail_first && tail_first < L && (op.kind == K::TailBlob) == lds, "tail op");
        bottom++;
        break;
      case K::CoarsestSweeps:
        reads(i);
        check(i == L - 1 && tail_first == L, "coarsest sweeps only without a tail, on the last level");
        sweeps[i] += 10;
        bottom++;
        break;
      case K::Prolong:
        check(bottom == 1 && sweeps[i] == 1, "prolongation after the bottom, before the post-smoother");
        break;
      case K::PostSmooth:
      case K::PostSmoothProlong:
        reads(i);
        check(bottom == 1, "post-smoother before the bottom");
        check(op.kind == K::PostSmooth || (lv[i].fused_prolong && !lv[i + 1].dist), "fused prolongation where flagged");
        sweeps[i]++;
        break;
      case K::ProlongSmoothPair:
        reads(i);
        reads(i - 1);
        check(bottom == 1 && i >= 1 && lv[i].up_pair, "up-leg pair without its flag");
        check(!in_pair_up[i] && !in_pair_up[i - 1], "up-leg pairs overlap");
        in_pair_up[i] = in_pair_up[i - 1] = 1;
        sweeps[i]++;
        sweeps[i - 1]++;
        break;
    }
  }
  check(bottom == 1, "exactly one bottom op");
  for (int l = 0; l < L; ++l) {
    if (l < down) check(sweeps[l] == 2, "a level above the tail is swept twice (even: ping-pong parity)");
    if (l <= down) check(rhs[l] == 1, "every level's rhs produced exactly once");
    if (l >= tail_first) check(sweeps[l] == 0, "a tail level swept outside the tail op");
  }
  if (tail_first == L) check(sweeps[L - 1] == 10, "ten coarsest sweeps");
}

// The level layout rules (RowWindow, level_ghosts, level_shape,
// transfer_bounds) on hierarchy H, rank by rank: its levels of more than rep
// rows from level 0 on are row-partitioned, as in Solver::build_amg_host.
// tops: the ranks' cell topologies (level 0's window).  Returns the number of
// row-partitioned levels.
int check_layout(const std::vector<cfd2::AmgHostLevel>& H, int R, uint64_t rep,
                 const std::vector<cfd2::Topology>& tops) {
  const int L = (int)H.size();
  int g = L;
  for (int l = 1; l < L; ++l)
    if (H[l].A.rows <= rep) {
      g = l;
      break;
    }
  auto ghosts_of = [&](int l, int q, std::vector<uint32_t>& gh) {
    const uint64_t C0 = H[l].part[q], C1 = H[l].part[q + 1];
    const cfd2::AmgHostLevel* F = l > 0 ? &H[l - 1] : nullptr;
    return cfd2::level_ghosts(C0, C1, H[l].A.row.data() + C0, (uint32_t)(C1 - C0), H[l].A.col.data(),
                              F ? F->agg.data() + F->part[q] : nullptr, F ? F->part[q + 1] - F->part[q] : 0, gh);
  };
  auto direct_shape = [](const cfd2::HostCsr& A, uint64_t C0, uint32_t n, const cfd2::RowWindow* w) {
    cfd2::LevelShape s;
    for (uint32_t i = 0; i < n; ++i) {
      int off = 0;
      for (uint32_t k = A.row[C0 + i]; k < A.row[C0 + i + 1]; ++k) {
        if (A.col[k] == C0 + i) continue;
        ++off;
        const int64_t d = (int64_t)(w ? w->rel(A.col[k]) : (int32_t)A.col[k]) - (int64_t)i;
        if (d < -32768 || d > 32767) s.small_delta = false;
      }
      s.wmax = std::max(s.wmax, off);
    }
    return s;
  };
  for (int l = 0; l < L; ++l) {
    const cfd2::HostCsr& A = H[l].A;
    if (l >= g) {  // replicated: global numbering, no window
      const cfd2::LevelShape s = cfd2::level_shape(A.row.data(), A.col.data(), (uint32_t)A.rows, 0, nullptr);
      const cfd2::LevelShape d = direct_shape(A, 0, (uint32_t)A.rows, nullptr);
      check(s.wmax == d.wmax && s.small_delta == d.small_delta, "level_shape of a replicated level");
      continue;
    }
    for (int q = 0; q < R; ++q) {
      const uint64_t C0 = H[l].part[q], C1 = H[l].part[q + 1];
      const uint32_t n = (uint32_t)(C1 - C0);
      // level_ghosts against a brute-force set
      std::vector<uint32_t> gh;
      const uint32_t glo = ghosts_of(l, q, gh);
      std::vector<char> in(A.rows, 0);
      for (uint64_t i = C0; i < C1; ++i)
        for (uint32_t k = A.row[i]; k < A.row[i + 1]; ++k) in[A.col[k]] = 1;
      if (l > 0)
        for (uint64_t i = H[l - 1].part[q]; i < H[l - 1].part[q + 1]; ++i) in[H[l - 1].agg[i]] = 1;
      std::vector<uint32_t> brute;
      uint32_t below = 0;
      for (uint64_t c = 0; c < A.rows; ++c)
        if (in[c] && (c < C0 || c >= C1)) {
          brute.push_back((uint32_t)c);
          below += c < C0;
        }
      check(gh == brute && glo == below, "level_ghosts differs from the brute-force set");
      // rel: monotone in the global id, onto [-glo, 0) u [0, n) u [npad, npad + ghi)
      const cfd2::RowWindow w(C0, C1, gh, glo);
      check(w.n() == n && w.ghi() == gh.size() - glo && w.npad % 64 == 0 && w.npad >= n && w.npad < n + 64, "window");
      std::vector<uint32_t> ids(gh.begin(), gh.begin() + glo);
      for (uint64_t c = C0; c < C1; ++c) ids.push_back((uint32_t)c);
      ids.insert(ids.end(), gh.begin() + glo, gh.end());
      int64_t prev = -(int64_t)glo - 1;
      for (size_t t = 0; t < ids.size(); ++t) {
        const int64_t r = w.rel(ids[t]);
        check(r > prev, "rel not strictly increasing in the global id");
        check((r >= -(int64_t)glo && r < (int64_t)n) || (r >= w.npad && r < (int64_t)w.npad + w.ghi()),
              "rel outside the window's local ranges");
        check((r < 0) == (t < glo) && (r >= (int64_t)w.npad) == (t >= glo + n), "rel range of a ghost / owned row");
        if (l == 0) check(r == tops[q].rel(ids[t]), "rel differs from Topology::rel on level 0");
        prev = r;
      }  // strictly increasing, ids.size() values inside a union of ids.size() integers: a bijection
      if (l == 0) check(gh == tops[q].ghost && glo == tops[q].glo && w.npad == tops[q].npad, "level 0 window");
      uint64_t stranger = A.rows;  // past the level; else the first row that is neither owned nor a ghost
      for (uint64_t c = 0; c < A.rows && stranger == A.rows; ++c)
        if (!in[c] && (c < C0 || c >= C1)) stranger = c;
      for (uint64_t c : {stranger, (uint64_t)A.rows}) {
        bool threw = false;
        try {
          (void)w.rel(c);
        } catch (const std::logic_error&) {
          threw = true;
        }
        check(threw, "rel of a row that is neither owned nor a ghost must throw");
      }
      // level_shape against a direct scan
      const cfd2::LevelShape s = cfd2::level_shape(A.row.data() + C0, A.col.data(), n, C0, &w);
      const cfd2::LevelShape d = direct_shape(A, C0, n, &w);
      check(s.wmax == d.wmax && s.small_delta == d.small_delta, "level_shape differs from a direct scan");
      // transfer_bounds over this rank's local P and R
      if (!H[l].has_op) continue;
      const bool next_dist = l + 1 < g;
      std::vector<uint32_t> ngh;
      const uint32_t nglo = next_dist ? ghosts_of(l + 1, q, ngh) : 0;
      const uint64_t I0 = H[l + 1].part[q], I1 = H[l + 1].part[q + 1];
      const cfd2::RowWindow nw(I0, I1, ngh, nglo);
      const uint32_t nc = (uint32_t)(I1 - I0);
      std::vector<uint32_t> agg(w.npad, 0), r_row(nc + 1), r_col;
      for (uint32_t i = 0; i < n; ++i) agg[i] = next_dist ? (uint32_t)nw.rel(H[l].agg[C0 + i]) : H[l].agg[C0 + i];
      for (uint32_t I = 0; I <= nc; ++I) r_row[I] = H[l].r_row[I0 + I] - H[l].r_row[I0];
      for (uint32_t k = H[l].r_row[I0]; k < H[l].r_row[I1]; ++k) {
        const int32_t lf = w.rel(H[l].r_col[k]);
        check(lf >= 0, "aggregate member below its seed's rank");
        r_col.push_back((uint32_t)lf);
      }
      const cfd2::TransferBounds tb = cfd2::transfer_bounds(r_row, r_col, agg, n, nc, next_dist);
      check(tb.rc_hi <= nc && tb.pf_lo <= n, "transfer bounds range");
      for (uint32_t I = 0; I < nc; ++I) {
        bool ghost = false;
        for (uint32_t k = r_row[I]; k < r_row[I + 1]; ++k) ghost = ghost || r_col[k] >= n;
        if (I < tb.rc_hi) check(!ghost, "an aggregate below rc_hi has a ghost member");
        if (I == tb.rc_hi) check(ghost, "aggregate rc_hi has only owned members");
      }
      check(tb.pf_lo % 4 == 0 || tb.pf_lo == n, "pf_lo neither a multiple of 4 nor the row count");
      if (!next_dist) check(tb.pf_lo == 0, "pf_lo into a replicated level");
      for (uint32_t i = tb.pf_lo; i < n && next_dist; ++i)
        check((int32_t)agg[i] >= 0 && agg[i] < nc, "a fine row at or above pf_lo belongs to a foreign aggregate");
    }
  }
  return g;
}

void run(const char* name, const cfd2::Mesh& m) {
  const cfd_mesh_view v = view_of(m);
  const uint32_t n = m.num_cells();
  for (int R = 1; R <= 4 && (uint32_t)R <= cfd2::red_geom(n).nseg; ++R) {
    const auto starts = cfd2::partition_starts(n, R);
    uint64_t rows = 0, nnz = 0, sends = 0, recvs = 0, reg_rows = 0;
    std::vector<cfd2::Topology> tops(R);
    for (int r = 0; r < R; ++r) {
      cfd2::Topology& t = tops[r];
      cfd2::build_topology(v, t, (uint32_t)starts[r], (uint32_t)starts[r + 1]);
      const cfd2::HaloPlan p =
          cfd2::build_halo_plan(starts, r, t.srow.data(), t.N, t.scol.data(), t.ghost, t.glo, t.npad);
      rows += t.N;
      nnz += t.scol.size();
      // aligned-slot coupled ELL: every CSR entry in its own, increasing slot,
      // with its column there; slots in use and gaps as the mask says
      for (uint32_t i = 0; i < t.N; ++i) {
        const uint32_t a = t.srow[i], len = t.srow[i + 1] - a;
        uint32_t on = 0;
        int prev = -1;
        for (uint32_t q = 0; q < len; ++q) {
          const int s = t.tslot[a + q];
          check(s > prev && s < t.ws, "aligned slots must increase inside the ELL width");
          check(t.tcol[(size_t)s * t.ld + i] == t.rel(t.scol[a + q]), "aligned slot holds its column");
          on |= 1u << s;
          prev = s;
        }
        const uint32_t used = t.tlg[i] & 0x7Fu, gap = t.tlg[i] >> 8;
        check(used == (uint32_t)prev + 1 && (gap | on) == (1u << used) - 1u && !(gap & on), "slot mask");
        check(t.tslot[a + t.ell_drank[i]] == t.tdrank8[i], "diagonal slot");
        bool all_modal = true;
        for (int r = 0; r < t.ws; ++r) {
          const int32_t c = t.tcol[(size_t)r * t.ld + i];
          check(c >= -(int32_t)t.glo && c < (int32_t)(t.npad + t.ghi), "virtual columns inside the vectors");
          if (r >= (int)t.tmode.size() || c != (int32_t)i + t.tmode[r]) all_modal = false;
        }
        // regular row (the kernels derive its columns): flagged iff every slot
        // holds row + tmode[slot] (aligned-slot layout only)
        const bool typed = t.ws <= 8;
        check(((t.tlg[i] & 0x80u) != 0) == (typed && all_modal), "regular-row flag");
        if (t.tlg[i] & 0x80u) reg_rows++;
      }
      for (const auto& h : p.peers) {
        sends += h.send_cnt;
        recvs += h.recv_cnt;
      }
    }
    check(rows == n, "rows do not add up");
    check(sends == recvs, "halo sends != receives");
    // host AMG hierarchy of a synthetic SPD-like matrix on the global pattern
    cfd2::Topology g;
    cfd2::build_topology(v, g);
    cfd2::HostCsr A;
    A.rows = A.cols = n;
    A.row = g.srow;
    A.col = g.scol;
    A.val.resize(g.scol.size());
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t k = g.srow[i]; k < g.srow[i + 1]; ++k)
        A.val[k] = g.scol[k] == i ? (float)(g.srow[i + 1] - g.srow[i]) : -1.0f;
    const auto H = cfd2::build_amg_hierarchy(A, 20, starts);
    check(!H.empty() && H[0].A.rows == n, "empty hierarchy");
    {  // partition-aware mode: no aggregate of a partitioned level straddles two parts
      const auto HL = cfd2::build_amg_hierarchy(A, 20, starts, true, 40);
      for (size_t l = 0; l + 1 < HL.size() && HL[l].A.rows > 40; ++l)
        for (int q = 0; q < R; ++q)
          for (uint64_t i = HL[l].part[q]; i < HL[l].part[q + 1]; ++i)
            check(HL[l].agg[i] >= HL[l + 1].part[q] && HL[l].agg[i] < HL[l + 1].part[q + 1],
                  "partition-aware aggregate straddles ranks");
      check_layout(HL, R, 40, tops);
    }
    {  // the level layout rules, levels of more than 40 rows row-partitioned
      const int g = check_layout(H, R, 40, tops);
      check(g >= 2, "fewer than two row-partitioned levels");
      std::printf("%s: %d rank(s): level layout rules on %d row-partitioned levels of %zu: ok\n", name, R, g,
                  H.size());
    }
    for (size_t l = 0; l + 1 < H.size(); ++l)
      check(H[l].has_op && H[l + 1].A.rows == H[l].nc, "level sizes");
    // down-leg pair partitions (k_amg_resrestrict_pair) of every level pair
    // with a coarser level, at the kernel's capacity and at a small one
    for (size_t l = 0; l + 2 < H.size(); ++l)
      for (uint32_t cap : {1024u, 96u}) {
        const cfd2::HostCsr& M = H[l + 1].A;
        const uint32_t nm = (uint32_t)M.rows;
        std::vector<uint32_t> mrow(nm + 1, 0), mcol;
        for (uint32_t g = 0; g < nm; ++g) {
          for (uint32_t k = M.row[g]; k < M.row[g + 1]; ++k)
            if (M.col[k] != g) mcol.push_back(M.col[k]);
          mrow[g + 1] = (uint32_t)mcol.size();
        }
        cfd2::PairPartition pp;
        if (!cfd2::build_pair_partition(H[l].r_row, H[l].r_col, H[l + 1].r_row, H[l + 1].r_col, mrow, mcol, cap, pp))
          continue;  // an aggregate alone over the capacity: no pair here
        std::vector<int> owner(nm, -1);
        const uint32_t nb = (uint32_t)pp.jb.size() - 1;
        check(pp.jb.back() == H[l + 1].nc && pp.sb.size() == nb + 1, "pair partition blocks");
        for (uint32_t b = 0; b < nb; ++b) {
          const uint32_t m0 = H[l + 1].r_row[pp.jb[b]], m1 = H[l + 1].r_row[pp.jb[b + 1]];
          const uint32_t s0 = pp.sb[b], s1 = pp.sb[b + 1];
          check(s1 - s0 <= cap && pp.fo[s1] - pp.fo[s0] <= cap && m1 - m0 <= s1 - s0, "pair block capacity");
          std::vector<int> in_s(nm, -1);
          for (uint32_t q = s0; q < s1; ++q) {
            check(in_s[pp.s[q]] < 0, "pair S row twice");
            in_s[pp.s[q]] = (int)(q - s0);
            const uint32_t g = pp.s[q];
            check(pp.fo[q + 1] - pp.fo[q] == H[l].r_row[g + 1] - H[l].r_row[g], "pair member count");
            for (uint32_t e = 0; e < pp.fo[q + 1] - pp.fo[q]; ++e)
              check(pp.f[pp.fo[q] + e] == H[l].r_col[H[l].r_row[g] + e], "pair members in R order");
          }
          for (uint32_t q = 0; q < m1 - m0; ++q) {
            const uint32_t g = pp.s[s0 + q];
            check(g == H[l + 1].r_col[m0 + q], "pair owned rows in R order");
            check(owner[g] < 0, "pair row owned twice");
            owner[g] = (int)b;
            for (uint32_t e = mrow[g]; e < mrow[g + 1]; ++e)
              check(in_s[mcol[e]] >= 0 && pp.lc[e] == (uint16_t)in_s[mcol[e]], "pair local column");
          }
          for (uint32_t q = m1 - m0; q < s1 - s0; ++q) {  // ring rows: columns of owned rows
            bool used = false;
            const uint32_t c = pp.s[s0 + q];
            for (uint32_t r = 0; r < m1 - m0 && !used; ++r) {
              const uint32_t g = pp.s[s0 + r];
              for (uint32_t e = mrow[g]; e < mrow[g + 1]; ++e) used = used || mcol[e] == c;
            }
            check(used, "pair ring row not a column of an owned row");
          }
        }
        for (uint32_t g = 0; g < nm; ++g) check(owner[g] >= 0, "pair row not owned");
      }
    // up-leg pair partitions (k_amg_prolong_smooth_pair): fine level l, coarse l + 1
    for (size_t l = 0; l + 1 < H.size(); ++l)
      for (uint32_t rows : {256u, 64u}) {
        const cfd2::HostCsr& Fm = H[l].A;
        const uint32_t nf = (uint32_t)Fm.rows, nc = H[l].nc;
        std::vector<uint32_t> frow(nf + 1, 0), fcol;
        for (uint32_t g = 0; g < nf; ++g) {
          for (uint32_t k = Fm.row[g]; k < Fm.row[g + 1]; ++k)
            if (Fm.col[k] != g) fcol.push_back(Fm.col[k]);
          frow[g + 1] = (uint32_t)fcol.size();
        }
        cfd2::UpPairPartition up;
        if (!cfd2::build_up_pair_partition(frow, fcol, H[l].agg, nc, rows, 1024, up)) continue;
        const uint32_t nb = (nf + rows - 1) / rows;
        check(up.tb.size() == nb + 1, "up pair blocks");
        for (uint32_t b = 0; b < nb; ++b) {
          const uint32_t t0 = up.tb[b], t1 = up.tb[b + 1];
          for (uint32_t q = t0 + 1; q < t1; ++q) check(up.t[q - 1] < up.t[q], "up pair T ascending");
          for (uint32_t f = b * rows; f < std::min(nf, (b + 1) * rows); ++f) {
            check(up.t[t0 + up.lto[f]] == H[l].agg[f], "up pair own aggregate");
            for (uint32_t e = frow[f]; e < frow[f + 1]; ++e)
              check(up.t[t0 + up.lt[e]] == H[l].agg[fcol[e]], "up pair column aggregate");
          }
        }
      }
    for (size_t l = 0; l < H.size(); ++l) {  // coarse rows follow their seeds: a partition in rank order
      check(H[l].part.size() == (size_t)R + 1 && H[l].part[0] == 0 && H[l].part[R] == H[l].A.rows, "level partition");
      for (int q = 0; q < R; ++q) check(H[l].part[q] <= H[l].part[q + 1], "level partition order");
    }
    {  // V-cycle schedules over this hierarchy: its big levels row-partitioned when R > 1
      const int L = (int)H.size();
      std::vector<cfd2::VcLevel> lv(L);
      int g = 0;  // first replicated level
      for (int l = 0; l < L; ++l) {
        lv[l].dist = R > 1 && H[l].A.rows > 200;
        if (lv[l].dist) g = l + 1;
        lv[l].fused_rr = !lv[l].dist && l + 1 < L && l % 3 != 2;  // some levels keep the two kernels
        lv[l].fused_prolong = !lv[l].dist;
      }
      check_schedule(lv, L, false);  // no tail, no pairs
      for (int l = 0; l < L; ++l) {  // every adjacent pair of replicated levels flagged
        lv[l].down_pair = !lv[l].dist;
        lv[l].up_pair = l >= 1 && !lv[l - 1].dist;
      }
      check_schedule(lv, L, false);
      const int mid = std::max({g, 1, L / 2});  // tail from a middle level, either kind
      check_schedule(lv, mid, true);
      check_schedule(lv, mid, false);
      std::printf("%s: %d rank(s): V-cycle schedules over %d levels (%d row-partitioned), tail from %d: ok\n", name, R,
                  L, g, mid);
    }
    std::printf("%s: %u cells, %d rank(s): nnz %llu, halo %llu, regular coupled rows %llu, %zu AMG levels: ok\n",
                name, n, R, (unsigned long long)nnz, (unsigned long long)sends, (unsigned long long)reg_rows,
                H.size());
  }
}

}  // namespace

int main() {
  try {
    cfd2::Geometry step{cfd2::kBackwardsStep, {2.0, 0.5, 1.0, 0.5}};
    cfd2::Mesh a = cfd2::generate_cut_cell_mesh(step, 0.05, 0.05, 1.2, 2.0, 1.0);
    a.smooth(step, 0.3, 10);
    cfd2::Geometry chan{cfd2::kChannelWithObstacle, {3.0, 1.0, 1.0, 0.5, 0.2}};
    cfd2::Mesh b = cfd2::generate_voronoi_mesh(chan, 0.04, 0.12, 1.2, 3.0, 1.0, 21);
    cfd2::Mesh c = cfd2::generate_delaunay_mesh(chan, 0.04, 0.12, 1.2, 3.0, 1.0, 22);
    run("cut-cell step", a);
    run("voronoi channel", b);
    run("delaunay channel", c);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
