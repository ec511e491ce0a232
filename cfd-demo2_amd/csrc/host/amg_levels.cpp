// The AMG level layout in device memory, written once for the three setups
// (build_amg_host below; device_levels and build_amg_device_dist in
// amg_device.cpp), which must produce byte-identical levels
// (amg_level_digest; tests/test_gpu_parity.py, tests/test_gpu_dist.py).  The
// GPU-free rules are RowWindow, level_ghosts and level_shape (dist.hpp) and
// transfer_bounds (amg_setup.cpp); the Solver members here turn them into
// device memory.  A builder decides only where a level's pattern and values
// come from, how the aggregation runs and how the coarse rows are filled.
// Also the hierarchy's lifetime: ensure_amg, drop_amg.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "solver_impl.hpp"

namespace cfd2 {

float* Solver::zeroed(size_t cnt) {
  float* p = arena.alloc<float>(cnt + 64);
  CFD_HIP(hipMemsetAsync(p, 0, (cnt + 64) * sizeof(float), stream));
  return p;
}

bool Solver::any_rank(bool mine) {
  for (uint64_t f : allgather_u64(mine ? 1 : 0))
    if (f) return true;
  return false;
}

void Solver::set_level_header(AmgGpuLevel& G, uint32_t n, uint32_t stride, const LevelShape& shape, uint64_t nnz) {
  G.nnz = nnz;
  G.npad = stride;  // (a row-partitioned level: its window's npad, the same number)
  G.wide = shape.wmax > amg_wide_limit;
  G.dev.n = n;
  G.dev.r0 = 0;
  G.dev.r1 = n;
  G.dev.stride = stride;
  G.dev.w = shape.wmax;
  G.dev.use16 = shape.small_delta ? 1 : 0;
}

void Solver::alloc_level_image(AmgGpuLevel& G) {
  AmgLevelDev& d = G.dev;
  const uint32_t st = d.stride;
  const size_t slots = (size_t)std::max(d.w, 1) * st;
  d.val = G.img.val = arena.alloc<float>(slots);
  d.col16 = G.img.col16 = d.use16 ? arena.alloc<int16_t>(slots) : nullptr;
  d.col32 = G.img.col32 = d.use16 ? nullptr : arena.alloc<int32_t>(slots);
  d.len = G.img.len = arena.alloc<uint8_t>(st);
  d.drank = G.img.drank = arena.alloc<uint8_t>(st);
  d.dv = G.img.dv = arena.alloc<float>(st);
  d.de = G.img.de = arena.alloc<float>(st);
}

void Solver::pack_level(const SetupMatrix& src, AmgGpuLevel& G) {
  const AmgLevelDev& d = G.dev;
  const AmgGpuLevel::Image& m = G.img;
  launch_amg_pack(src, d.n, d.stride, d.w, d.use16, m.val, m.col16, m.col32, m.len, m.drank, m.dv, m.de, stream);
  CFD_HIP(hipGetLastError());
}

// Host-built image of the rows of A that `win` owns (nullptr: every row,
// global numbering), off-diagonal columns as local indices; see AmgLevelDev.
void Solver::level_image(const HostCsr& A, const RowWindow* win, AmgGpuLevel& G) {
  const uint64_t r0 = win ? win->c0 : 0;
  const uint32_t n = win ? win->n() : (uint32_t)A.rows;
  const uint32_t st = (n + 63) & ~63u;  // padded row count (16-byte row groups)
  const LevelShape shape = level_shape(A.row.data() + r0, A.col.data(), n, r0, win);
  if (shape.wmax > 65535) throw std::invalid_argument("AMG level row wider than 65535 entries (unsupported)");
  const bool small_delta = shape.small_delta;
  const uint32_t w1 = (uint32_t)std::max(shape.wmax, 1);
  const size_t slots = (size_t)w1 * st;
  std::vector<uint8_t> len(st, 0), drank(st, 0);
  std::vector<uint16_t> len16(st, 0), drank16(st, 0);
  std::vector<float> dv(st, 0.0f), de(st, 1.0f);
  std::vector<float> val(slots, 0.0f);
  std::vector<int16_t> col16(small_delta ? slots : 0, 0);
  std::vector<int32_t> col32(small_delta ? 0 : slots, 0);
  for (uint32_t i = 0; i < st; ++i) {
    uint32_t r = 0;
    if (i < n) {
      const uint64_t gi = r0 + i;
      uint32_t dr = 0;
      bool has = false;
      float diag = 1.0f, raw = 0.0f;
      for (uint32_t k = A.row[gi]; k < A.row[gi + 1]; ++k) {
        const uint32_t c = A.col[k];
        if (c == gi) {
          has = true;
          raw = A.val[k];
          diag = raw;
          dr = r;
          continue;
        }
        const int32_t lc = win ? win->rel(c) : (int32_t)c;
        const size_t o = (size_t)r * st + i;
        val[o] = A.val[k];
        if (small_delta)
          col16[o] = (int16_t)((int64_t)lc - (int64_t)i);
        else
          col32[o] = lc;
        ++r;
      }
      if (!has) dr = r;  // no diagonal entry: raw diag contributes nothing (dv = 0)
      if (std::fabs(diag) < 1e-14f) diag = 1.0f;  // amg.wgsl:46
      len[i] = (uint8_t)std::min(r, 255u);
      drank[i] = (uint8_t)std::min(dr, 255u);
      len16[i] = (uint16_t)r;
      drank16[i] = (uint16_t)dr;
      dv[i] = raw;
      de[i] = diag;
    }
    // padding slots / rows: value 0, column = the row itself (allocated, zeroed)
    if (!small_delta)
      for (; r < w1; ++r) col32[(size_t)r * st + i] = (int32_t)i;
  }
  set_level_header(G, n, st, shape, A.row[r0 + n] - A.row[r0]);
  G.dev.val = arena.upload(val, stream);
  G.dev.col16 = small_delta ? arena.upload(col16, stream) : nullptr;
  G.dev.col32 = small_delta ? nullptr : arena.upload(col32, stream);
  G.dev.len = arena.upload(len, stream);
  G.dev.drank = arena.upload(drank, stream);
  G.dev.dv = arena.upload(dv, stream);
  G.dev.de = arena.upload(de, stream);
  G.dev.len16 = G.wide ? arena.upload(len16, stream) : nullptr;
  G.dev.drank16 = G.wide ? arena.upload(drank16, stream) : nullptr;
}

// The three vector layouts.  Level 0's x and b are bound per cycle (p_sol,
// temp_p); on a row-partitioned run its xt and r are cell vectors too.  A
// row-partitioned coarse level keeps its lower ghosts below the owned base and
// its upper ghosts from npad on; a replicated (or single-GPU) level has no ghosts.
void Solver::alloc_level_vectors(AmgGpuLevel& G, int li) {
  if (G.dist && li == 0) {
    if (G.glo != topo.glo || G.ghi != topo.ghi || G.npad != topo.npad)
      throw std::logic_error("AMG level 0 ghosts differ from the cell ghosts");
    G.xt = valloc<float>(1);
    G.r = valloc<float>(1);
  } else if (G.dist) {
    const uint32_t sh = (G.glo + 63) & ~63u;
    const size_t cnt = (size_t)sh + G.npad + G.ghi;
    G.x = zeroed(cnt) + sh;
    G.xt = zeroed(cnt) + sh;
    G.b = zeroed(cnt) + sh;
    G.r = zeroed(cnt) + sh;
  } else {
    G.xt = zeroed(G.npad);
    G.r = zeroed(G.npad);
    if (li > 0) {
      G.x = zeroed(G.npad);
      G.b = zeroed(G.npad);
    }
  }
}

void Solver::upload_transfer(AmgGpuLevel& G, const std::vector<uint32_t>& agg, const std::vector<uint32_t>& r_row,
                             const std::vector<uint32_t>& r_col) {
  std::vector<uint32_t> aggp(G.dev.stride, 0);
  std::copy(agg.begin(), agg.begin() + G.dev.n, aggp.begin());
  std::vector<int32_t> m4;
  build_r_m4(r_row, r_col, m4);
  G.dev.agg = arena.upload(aggp, stream, kAggSlack);
  G.dev.r_row = arena.upload(r_row, stream);
  G.dev.r_col = arena.upload(r_col, stream);
  G.dev.r_m4 = reinterpret_cast<const int4*>(arena.upload(m4, stream));
  G.dev.nc = (uint32_t)r_row.size() - 1;
}

bool Solver::galerkin_count(const SetupMatrix& A, const uint32_t* gal_agg, const uint32_t* r_row,
                            const uint32_t* r_col, uint32_t nagg, bool collective, std::vector<uint32_t>& rowptr) {
  DevTmp<uint32_t> d_cnt(nagg);
  launch_galerkin(A, gal_agg, r_row, r_col, nagg, d_cnt.p, nullptr, nullptr, nullptr, amg_setup_flag, stream);
  CFD_HIP(hipGetLastError());
  rowptr.assign((size_t)nagg + 1, 0);
  uint32_t flag = 0;
  if (nagg)
    CFD_HIP(hipMemcpyAsync(rowptr.data() + 1, d_cnt.p, (size_t)nagg * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           stream));
  CFD_HIP(hipMemcpyAsync(&flag, amg_setup_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  sync();
  if (collective ? any_rank(flag != 0) : flag != 0) return false;
  for (uint32_t I = 0; I < nagg; ++I) rowptr[I + 1] += rowptr[I];
  return true;
}

// Unconditional slot loads + vector gathers (MODE 1, amg_rows.hpp
// gather_group) where the rows fill the ELL width (level 0, the face stencil;
// the first coarse levels of the face-stencil meshes: mean off-diagonal count
// >= 3/4 of the width; C2 A/B: level-1 smoother 55.0 -> 50.2 us, level 2
// 15.1 -> 12.3) and on the small latency-bound levels; predicated loads on the
// ragged big coarse levels, whose row lengths vary (same-box A/B at C2: level 1
// smoother 58 vs 66 us, small-level residual 6 vs 8.5 us).
void Solver::set_amg_full_policy(AmgGpuLevel& G, int li) {
  const char* fe = knob(Knob::AmgFull);
  const double n = std::max<double>(G.dev.n, 1.0);
  const double offd = ((double)G.nnz - n) / n;  // mean off-diagonals per row
  const bool regular = G.dev.w > 0 && offd >= 0.75 * G.dev.w;
  G.dev.full = fe ? (fe[0] == '1') : (li == 0 || regular || G.dev.n <= (1u << 19));
}

// Drop the hierarchy (its device memory included); the next AMG solve builds
// a new one from the matrix of that moment (or from a loaded source).
void Solver::drop_amg() {
  CFD_HIP(hipSetDevice(device));
  sync();
  drop_graphs();  // they hold the hierarchy's pointers
  levels.clear();
  d_tail = nullptr;
  tail_blob_first = -1;
  d_tail_blob = nullptr;
  d_tail_desc = nullptr;
  tail_blob_words = tail_vec_floats = 0;
  amg_refresh.clear();
  rr_pair.clear();  // their block images lived in amg_arena
  up_pair.clear();
  vc_plan.clear();
  amg_setup_flag = nullptr;
  amg_refresh_pending = false;
  amg_arena.release();
  amg_built = false;
  amg_setup_path = 0;
  amg_age = 0;
}

void Solver::ensure_amg() {
  if (amg_built) {
    if (amg_refresh_pending) {
      const Range range("amg refresh");
      refresh_amg();
      amg_refresh_pending = false;
      amg_age = 0;
    }
    return;
  }
  const Range range("amg setup");
  const bool timing = cfg.log_level >= 2 && rk == 0;
  const auto t_start = std::chrono::steady_clock::now();
  const char* se = knob(Knob::AmgSetup);
  if (se && std::strcmp(se, "host") && std::strcmp(se, "device") && std::strcmp(se, "rebuild"))
    throw std::invalid_argument(std::string("CFD_AMG_SETUP: expected device, host or rebuild, got ") + se);
  const bool device_setup = !(se && std::string(se) == "host");
  const char* how = "device";
  amg_setup_path = 2;
  const size_t slots_s = (size_t)topo.ws * topo.ld;
  if (!amg_src) amg_src = arena.alloc<float>(slots_s);
  const bool from_checkpoint = amg_src_loaded;  // then amg_age is the saved run's
  if (!from_checkpoint)  // keep the source matrix for cfd_state_save
    CFD_HIP(hipMemcpyAsync(amg_src, sval, slots_s * sizeof(float), hipMemcpyDeviceToDevice, stream));
  amg_src_loaded = false;
  // both setup paths read `sval`: point it at the source for the build; the
  // hierarchy's allocations go to amg_arena (arena swapped for the build)
  float* const live = sval;
  sval = amg_src;
  amg_arena.release();
  arena.swap(amg_arena);
  struct Restore {
    Solver* s;
    float* live;
    ~Restore() {
      s->sval = live;
      s->arena.swap(s->amg_arena);
    }
  } restore{this, live};
  if (!(device_setup && build_amg_device())) {
    how = "host";
    amg_setup_path = 1;
    levels.clear();
    arena.release();  // the device attempt's partial hierarchy
    build_amg_host();
  }
  finish_amg_schedule();
  sync();
  amg_built = true;
  if (!from_checkpoint) amg_age = 0;
  if (timing) {
    std::string pairs, ups;  // the pairs the schedule runs, either leg by ascending level
    for (const VcOp& op : vc_plan) {
      const std::string a = " " + std::to_string(op.level) + "+";
      if (op.kind == VcKind::ResRestrictPair) pairs += a + std::to_string(op.level + 1);
      if (op.kind == VcKind::ProlongSmoothPair) ups = a + std::to_string(op.level - 1) + ups;
    }
    std::fprintf(stderr,
                 "[amg setup] %s path: %d levels in %.3f s, tail from level %d (LDS image from level %d), "
                 "down-leg pairs:%s, up-leg pairs:%s\n",
                 how, (int)levels.size(),
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), tail_first,
                 tail_blob_first, pairs.empty() ? " none" : pairs.c_str(), ups.empty() ? " none" : ups.c_str());
  }
}

// Host AMG setup (fallback of build_amg_device, or CFD_AMG_SETUP=host;
// ensure_amg_resources, coupled_solver_fgmres.rs:174-209): read back the live
// scalar matrix, build the frozen hierarchy on the host (amg_setup.cpp), upload
// every level.  A distributed rank all-gathers the scalar matrix, builds the
// GLOBAL hierarchy (the one a single GPU builds, so results do not depend on
// the rank count) and keeps its rows of the levels with more than
// CFD_AMG_REPLICATE_ROWS rows (default kAmgReplicateRowsDefault); the small
// levels are replicated on every rank.
void Solver::build_amg_host() {
  const size_t ld = topo.ld;
  std::vector<float> ell((size_t)topo.ws * ld);
  CFD_HIP(hipMemcpyAsync(ell.data(), sval, ell.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  std::vector<float> own(topo.scol.size());
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t k = topo.srow[i]; k < topo.srow[i + 1]; ++k) own[k] = ell[(size_t)(k - topo.srow[i]) * ld + i];
  HostCsr A0;
  std::vector<AmgHostLevel> H;
  if (!dist()) {
    A0.rows = A0.cols = N;
    A0.row = topo.srow;
    A0.col = topo.scol;
    A0.val = std::move(own);
    H = build_amg_hierarchy(A0, kMaxAmgLevels, {}, false, 0, cfg.log_level >= 2);
  } else {
    // all-gather the global pattern and the values (row order = global order, rank by rank)
    const std::vector<uint64_t> nz = allgather_u64(topo.scol.size());
    std::vector<uint64_t> eoff(R + 1, 0);
    for (int q = 0; q < R; ++q) eoff[q + 1] = eoff[q] + nz[q];
    std::vector<size_t> roff(R + 1), coff(R + 1);
    for (int q = 0; q <= R; ++q) {
      roff[q] = starts[q] * sizeof(uint32_t);
      coff[q] = eoff[q] * sizeof(uint32_t);
    }
    const size_t nnz_all = eoff[R];
    std::vector<uint32_t> lens(NG, 0);
    for (uint32_t i = 0; i < N; ++i) lens[starts[rk] + i] = topo.srow[i + 1] - topo.srow[i];
    uint32_t* d_lens = arena.alloc<uint32_t>(NG);
    uint32_t* d_cols = arena.alloc<uint32_t>(nnz_all);
    float* d_vals = arena.alloc<float>(nnz_all);
    CFD_HIP(hipMemcpyAsync(d_lens, lens.data(), (size_t)NG * 4, hipMemcpyHostToDevice, stream));
    CFD_HIP(hipMemcpyAsync(d_cols + eoff[rk], topo.scol.data(), topo.scol.size() * 4, hipMemcpyHostToDevice, stream));
    CFD_HIP(hipMemcpyAsync(d_vals + eoff[rk], own.data(), own.size() * 4, hipMemcpyHostToDevice, stream));
    comm->allgatherv_inplace(d_lens, roff, stream);
    comm->allgatherv_inplace(d_cols, coff, stream);
    comm->allgatherv_inplace(d_vals, coff, stream);
    A0.rows = A0.cols = NG;
    A0.row.assign((size_t)NG + 1, 0);
    A0.col.resize(nnz_all);
    A0.val.resize(nnz_all);
    CFD_HIP(hipMemcpyAsync(lens.data(), d_lens, (size_t)NG * 4, hipMemcpyDeviceToHost, stream));
    CFD_HIP(hipMemcpyAsync(A0.col.data(), d_cols, nnz_all * 4, hipMemcpyDeviceToHost, stream));
    CFD_HIP(hipMemcpyAsync(A0.val.data(), d_vals, nnz_all * 4, hipMemcpyDeviceToHost, stream));
    sync();
    for (uint32_t i = 0; i < NG; ++i) A0.row[i + 1] = A0.row[i] + lens[i];
    H = build_amg_hierarchy(A0, kMaxAmgLevels, starts, amg_local, amg_replicate_rows(), cfg.log_level >= 2 && rk == 0);
  }
  const int L = (int)H.size();
  // distributed levels [0, amg_g): the rest are replicated (all of them on one GPU)
  amg_g = 0;
  if (dist()) {
    const uint64_t rep = amg_replicate_rows();
    amg_g = L;
    for (int li = 1; li < L; ++li)
      if (H[li].A.rows <= rep) {
        amg_g = li;
        break;
      }
  }
  // Ghost lists of every rank on the distributed levels (the halo plans need
  // both directions): the matrix columns outside the rank's rows, plus on a
  // coarse level the aggregates of the rank's finer rows that another rank
  // owns (an aggregate belongs to its seed's rank and may reach into the next
  // ranks: the prolongation reads those coarse values, the restriction the
  // fine residuals of members owned by the next ranks, which are matrix
  // neighbours of the seed and so already ghosts of the seed's rank).
  std::vector<std::vector<std::vector<uint32_t>>> ghosts(amg_g);
  std::vector<RowWindow> win(amg_g);  // this rank's rows of each distributed level
  for (int li = 0; li < amg_g; ++li) {
    const AmgHostLevel& HL = H[li];
    const AmgHostLevel* HF = li > 0 ? &H[li - 1] : nullptr;
    ghosts[li].resize(R);
#pragma omp parallel for schedule(dynamic, 1)
    for (int q = 0; q < R; ++q) {
      const uint64_t C0 = HL.part[q], C1 = HL.part[q + 1];
      const uint32_t glo = level_ghosts(C0, C1, HL.A.row.data() + C0, (uint32_t)(C1 - C0), HL.A.col.data(),
                                        HF ? HF->agg.data() + HF->part[q] : nullptr,
                                        HF ? HF->part[q + 1] - HF->part[q] : 0, ghosts[li][q]);
      if (q == rk) win[li] = RowWindow(C0, C1, ghosts[li][q], glo);
    }
  }
  levels.assign(L, AmgGpuLevel{});
  for (int li = 0; li < L; ++li) {
    const AmgHostLevel& HL = H[li];
    AmgGpuLevel& G = levels[li];
    const RowWindow* W = li < amg_g ? &win[li] : nullptr;  // else replicated (or single-GPU), global numbering
    G.nglob = HL.A.rows;
    G.part = HL.part;
    G.C0 = HL.part[rk];
    G.C1 = HL.part[rk + 1];
    level_image(HL.A, W, G);
    if (W) {
      G.dist = true;
      G.glo = W->glo;
      G.ghi = W->ghi();
      G.plan = build_halo_plan_lists(HL.part, rk, ghosts[li], G.glo, G.npad);
      interior_rows(HL.part, rk, HL.A.row.data() + G.C0, G.dev.n, HL.A.col.data(), G.plan.lo_end, G.plan.hi_begin);
      make_plan_buffers(G.plan, 1);
    }
    alloc_level_vectors(G, li);
    set_amg_full_policy(G, li);
    if (!HL.has_op) continue;
    // coarsening operators: P as an aggregate index per stored fine row
    // (signed local coarse index into a distributed next level, global id into
    // a replicated one), R = P^T rows of this rank's aggregates with local fine
    // members (owned, or ghosts of the next ranks)
    if (!W) {
      upload_transfer(G, HL.agg, HL.r_row, HL.r_col);
      continue;
    }
    const bool next_dist = li + 1 < amg_g;
    const uint32_t n = G.dev.n;
    std::vector<uint32_t> agg(n), r_row, r_col;
    for (uint32_t i = 0; i < n; ++i)
      agg[i] = next_dist ? (uint32_t)win[li + 1].rel(HL.agg[G.C0 + i]) : HL.agg[G.C0 + i];
    const uint64_t I0 = H[li + 1].part[rk], I1 = H[li + 1].part[rk + 1];
    r_row.resize(I1 - I0 + 1);
    for (uint64_t I = I0; I <= I1; ++I) r_row[I - I0] = HL.r_row[I] - HL.r_row[I0];
    r_col.assign(HL.r_col.begin() + HL.r_row[I0], HL.r_col.begin() + HL.r_row[I1]);
    for (auto& f : r_col) {
      const int32_t lf = W->rel(f);
      if (lf < 0) throw std::logic_error("AMG: aggregate member below its seed's rank");
      f = (uint32_t)lf;
    }
    const TransferBounds tb = transfer_bounds(r_row, r_col, agg, n, (uint32_t)(I1 - I0), next_dist);
    G.rc_hi = tb.rc_hi;
    G.pf_lo = tb.pf_lo;
    upload_transfer(G, agg, r_row, r_col);
  }
}

uint64_t Solver::amg_level_digest(int li) {
  if (li < 0 || li >= (int)levels.size()) throw std::invalid_argument("no such AMG level");
  CFD_HIP(hipSetDevice(device));
  const AmgLevelDev& d = levels[li].dev;
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  };
  auto dev = [&](const void* src, size_t bytes) {
    if (!src || !bytes) return;
    std::vector<unsigned char> tmp(bytes);
    CFD_HIP(hipMemcpyAsync(tmp.data(), src, bytes, hipMemcpyDeviceToHost, stream));
    sync();
    mix(tmp.data(), bytes);
  };
  const uint32_t hdr[6] = {d.n, d.stride, (uint32_t)d.w, (uint32_t)d.use16, d.nc, (uint32_t)levels[li].nnz};
  mix(hdr, sizeof(hdr));
  const size_t slots = (size_t)std::max(d.w, 1) * d.stride;
  dev(d.val, slots * 4);
  dev(d.col16, d.use16 ? slots * 2 : 0);
  dev(d.col32, d.use16 ? 0 : slots * 4);
  dev(d.len, d.stride);
  dev(d.drank, d.stride);
  dev(d.dv, (size_t)d.stride * 4);
  dev(d.de, (size_t)d.stride * 4);
  if (d.nc) {
    dev(d.agg, (size_t)d.stride * 4);
    std::vector<uint32_t> rr((size_t)d.nc + 1);
    CFD_HIP(hipMemcpyAsync(rr.data(), d.r_row, rr.size() * 4, hipMemcpyDeviceToHost, stream));
    sync();
    mix(rr.data(), rr.size() * 4);
    dev(d.r_col, (size_t)rr[d.nc] * 4);
  }
  return h;
}

}  // namespace cfd2
