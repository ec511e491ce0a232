// The AMG V-cycle of the HIP solver (linear_solver/amg.rs:666-770): what the
// setup decides after the hierarchy is built (fused forms, tail, pair images,
// the launch schedule), the cycle that runs the schedule, and the plain
// dispatch-by-dispatch cycle of the reference-semantics mode.  The schedule
// itself is plan_v_cycle (amg_setup.cpp); accounting.cpp prices it.
#include <algorithm>
#include <cstring>

#include "solver_impl.hpp"

namespace cfd2 {

// The last part of ensure_amg(), inside its arena swap: everything the cycle
// needs beyond the level images.
void Solver::finish_amg_schedule() {
  const int L = (int)levels.size();
  set_resrestrict_blocks();
  // post-smoothers with the prolongation fused (single-GPU / replicated
  // levels of at most CFD_AMG_FUSED_PROLONG_ROWS rows; 0: never)
  fuse_prolong_rows = knob_u64(Knob::AmgFusedProlongRows, 1ull << 20);
  // the tail form: blob<K> (default blob2), lds, global
  {
    const char* tf = knob(Knob::AmgTail);
    tail_form = 2;
    tail_blob_shift = 2;
    if (tf && std::strncmp(tf, "blob", 4) == 0) {
      if (tf[4]) tail_blob_shift = std::max(0, (int)std::strtol(tf + 4, nullptr, 10));
    } else if (tf && std::strcmp(tf, "lds") == 0) {
      tail_form = 1;
    } else if (tf && std::strcmp(tf, "global") == 0) {
      tail_form = 0;
    } else if (tf) {
      throw std::invalid_argument(std::string("CFD_AMG_TAIL: expected blob<K>, lds or global, got ") + tf);
    }
  }
  // replicated levels from `tail_first` down run inside one single-workgroup kernel
  const uint32_t tail_rows = (uint32_t)knob_u64(Knob::AmgTailRows, 4096u);
  const int lo = std::max(amg_g, 1);
  tail_first = L;
  while (tail_first > lo && levels[tail_first - 1].dev.n <= tail_rows) --tail_first;
  // wide levels (16-bit row lengths) run only in the one-workgroup tail kernels
  {
    int bad = -1;  // first wide level the row kernels would run (level 0 or a row-partitioned level)
    for (int li = 0; li < L; ++li)
      if (levels[li].wide) {
        if (li < lo)
          bad = li;
        else
          tail_first = std::min(tail_first, li);
        break;
      }
    // the width of a row-partitioned level is per rank: every rank throws together
    uint64_t any_bad = bad >= 0 ? 1 : 0;
    if (dist())
      for (uint64_t f : allgather_u64(any_bad)) any_bad |= f;
    if (any_bad)
      throw std::invalid_argument("AMG: rows wider than 255 entries on a level the row kernels run (level 0 or a "
                                  "row-partitioned level): unsupported layout");
  }
  std::vector<AmgTailLevel> tl(L);
  for (int li = 0; li < L; ++li) {
    tl[li].L = levels[li].dev;
    tl[li].x = levels[li].x;
    tl[li].xt = levels[li].xt;
    tl[li].b = levels[li].b;
    tl[li].r = levels[li].r;
  }
  d_tail = arena.upload(tl, stream);
  check_launch("AMG setup");
  if (tail_form == 2) {
    // The LDS image of the tail (matrices included) is the fast tail; when it
    // does not fit in one CU's LDS, up to tail_blob_shift (CFD_AMG_TAIL=blob<K>,
    // default 2) more levels run with the row kernels so that it does (C1: the
    // 3.9 k-row level).
    const int t0 = tail_first;
    for (int t = t0; t < std::min(L, t0 + 1 + tail_blob_shift) && tail_blob_first < 0; ++t) {
      if (t > t0 && levels[t - 1].wide) break;  // wide levels run only in the tail kernels
      build_tail_blob(t);
      if (tail_blob_first >= 0) tail_first = t;
    }
  }
  // tail_first only moved down to `lo`, or up (wide clamp from `lo` on, blob shift)
  if (tail_first < lo || tail_first > L) throw std::logic_error("AMG setup: tail_first outside [max(amg_g, 1), L]");
  build_rr_pairs();
  std::vector<VcLevel> lv(L);
  for (int li = 0; li < L; ++li)
    lv[li] = {levels[li].dist, levels[li].dev.rr_agg != 0, rr_pair[li].nblocks != 0, up_pair[li].nblocks != 0,
              fused_prolong(li)};
  vc_plan = plan_v_cycle(lv, tail_first, tail_first == tail_blob_first);
}

// Aggregates per block of k_amg_resrestrict for the single-GPU / replicated
// levels with a coarse level and at most CFD_AMG_FUSED_RR_ROWS rows (default
// 2^18; distributed levels restrict ghost residuals and keep the two
// kernels): about 256 members per block, fewer aggregates while a block's
// members exceed its LDS capacity.  Its one-row-per-thread residual over
// permuted rows only pays on the latency-bound levels: same-box A/B
// (profiles/r03/ab_log.md) C2 level 0 129 vs 68 + 34 us, level 1 104 vs
// 56 + 13 us; C1 levels of 125 k rows and fewer 6-8 vs 10-11 us.
// CFD_AMG_FUSED_RR_ROWS=0 keeps the two kernels everywhere.
void Solver::set_resrestrict_blocks() {
  const uint64_t max_rows = knob_u64(Knob::AmgFusedRrRows, 1u << 18);
  for (AmgGpuLevel& G : levels) {
    AmgLevelDev& d = G.dev;
    d.rr_agg = 0;
    if (max_rows == 0 || G.dist || d.nc == 0 || d.n == 0 || d.n > max_rows || !d.r_row) continue;
    std::vector<uint32_t> rr((size_t)d.nc + 1);
    CFD_HIP(hipMemcpyAsync(rr.data(), d.r_row, rr.size() * 4, hipMemcpyDeviceToHost, stream));
    sync();
    uint32_t a = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(256, (uint64_t)256 * d.nc / d.n));
    for (; a >= 1; a /= 2) {
      uint32_t worst = 0;
      for (uint32_t I = 0; I < d.nc; I += a) worst = std::max(worst, rr[std::min(I + a, d.nc)] - rr[I]);
      if (worst <= kRRCap) break;
    }
    d.rr_agg = a;
  }
}

// Down-leg pairs (k_amg_resrestrict_pair): greedily from the top, two
// adjacent levels that both take k_amg_resrestrict and whose second level is
// pre-smoothed inside the V-cycle's down loop run as one launch.
void Solver::build_rr_pairs() {
  const int L = (int)levels.size();
  rr_pair.assign(L, AmgPairImage{});
  up_pair.assign(L, AmgUpPairImage{});
  pair_mode = (int)knob_u64(Knob::AmgFusedPair, 1);  // 0 off, 1 where cheap, 2 every candidate (tests)
  if (pair_mode == 0) return;
  const int down = v_cycle_down(tail_first, L);  // as plan_v_cycle: only levels the cycle runs are paired
  for (int i = 0; i + 1 < down;) {
    const AmgGpuLevel &F = levels[i], &M = levels[i + 1];
    const bool ok = !F.dist && !M.dist && !F.wide && !M.wide && F.dev.rr_agg && M.dev.rr_agg && M.dev.w >= 1;
    i += (ok && build_rr_pair(i)) ? 2 : 1;
  }
  // up-leg: from the bottom, post-smoothers of levels c and c - 1 that both
  // take the fused prolongation, fine level at most 2^18 rows
  for (int c = down - 1; c >= 1;) {
    const AmgGpuLevel &C = levels[c], &F = levels[c - 1];
    const bool ok = fused_prolong(c) && fused_prolong(c - 1) && !C.wide && !F.wide && F.dev.n <= (1u << 18) &&
                    F.dev.w >= 1 && C.dev.agg;
    c -= (ok && build_up_pair(c)) ? 2 : 1;
  }
}

bool Solver::level_csr(const AmgLevelDev& d, std::vector<uint32_t>& row, std::vector<uint32_t>& col,
                       std::vector<float>* val) {
  const uint32_t n = d.n, st = d.stride;
  const size_t slots = (size_t)std::max(d.w, 1) * st;
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) CFD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
  };
  std::vector<uint8_t> len8(d.len16 ? 0 : n);
  std::vector<uint16_t> len(n);  // a wide level keeps its true lengths in len16 (len holds min(., 255))
  std::vector<float> v(val ? slots : 0);
  std::vector<int16_t> c16(d.use16 ? slots : 0);
  std::vector<int32_t> c32(d.use16 ? 0 : slots);
  if (d.len16) d2h(len.data(), d.len16, (size_t)n * 2);
  else d2h(len8.data(), d.len, n);
  if (val) d2h(v.data(), d.val, slots * 4);
  if (d.use16) d2h(c16.data(), d.col16, slots * 2);
  else d2h(c32.data(), d.col32, slots * 4);
  sync();
  if (!d.len16) std::copy(len8.begin(), len8.end(), len.begin());
  row.assign((size_t)n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if ((int)len[i] > d.w) throw std::logic_error("AMG level image: a row longer than the level's width");
    row[i + 1] = row[i] + len[i];
  }
  col.resize(row[n]);
  if (val) val->resize(row[n]);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < len[i]; ++r) {
      const size_t o = (size_t)r * st + i;
      const int64_t c = d.use16 ? (int64_t)i + c16[o] : (int64_t)c32[o];
      if (c < 0 || c >= (int64_t)n) return false;
      col[row[i] + r] = (uint32_t)c;
      if (val) (*val)[row[i] + r] = v[o];
    }
  return true;
}

namespace {
// per-entry indices of a level_csr pattern, back in the level's slot layout
std::vector<uint16_t> to_slots(const AmgLevelDev& d, const std::vector<uint32_t>& row, const std::vector<uint16_t>& v) {
  std::vector<uint16_t> out((size_t)d.w * d.stride, 0);
  for (uint32_t g = 0; g < d.n; ++g)
    for (uint32_t k = row[g]; k < row[g + 1]; ++k) out[(size_t)(k - row[g]) * d.stride + g] = v[k];
  return out;
}
}  // namespace

// The up-leg pair image of levels (c, c - 1): blocks of kUpPairRows fine rows
// and the level-c rows T they need (kUpPairCap at most), with the T-local
// index of every fine slot's column aggregate.  Mode 1 pairs only while the
// blocks' T rows total at most 2.5x the level's rows (profiles/r06/ab_log.md,
// C1: levels 5+4 9.1 us against 7.5 + 6.3, in; 3+2 13.1 against 6.8 + 6.7,
// out).
bool Solver::build_up_pair(int c) {
  const AmgLevelDev &F = levels[c - 1].dev, &C = levels[c].dev;
  std::vector<uint32_t> agg(F.n), frow, fcol;
  CFD_HIP(hipMemcpyAsync(agg.data(), F.agg, (size_t)F.n * 4, hipMemcpyDeviceToHost, stream));
  if (!level_csr(F, frow, fcol)) return false;
  UpPairPartition up;
  if (!build_up_pair_partition(frow, fcol, agg, C.n, kUpPairRows, kUpPairCap, up)) return false;
  if (pair_mode < 2 && (double)up.t.size() > 2.5 * (double)C.n) return false;
  const std::vector<uint16_t> lt = to_slots(F, frow, up.lt);
  std::vector<uint16_t> lto(F.stride, 0);
  std::copy(up.lto.begin(), up.lto.begin() + F.n, lto.begin());
  AmgUpPairImage& P = up_pair[c];
  P.nblocks = (uint32_t)up.tb.size() - 1;
  P.tb = arena.upload(up.tb, stream);
  P.t = arena.upload(up.t, stream);
  P.lt = arena.upload(lt, stream);
  P.lto = arena.upload(lto, stream);
  sync();
  return true;
}

// The pair image of levels (i, i+1): blocks of level-(i+2) aggregates whose
// level-(i+1) rows (members + ring: S) and level-i members of S each fit
// kPairThreads.  False (no pair) when one aggregate alone does not fit.
bool Solver::build_rr_pair(int i) {
  const AmgLevelDev &F = levels[i].dev, &M = levels[i + 1].dev;
  const uint32_t nm = M.n, nc = M.nc;
  auto down_u32 = [&](const uint32_t* d, size_t n) {
    std::vector<uint32_t> h(n);
    CFD_HIP(hipMemcpyAsync(h.data(), d, n * 4, hipMemcpyDeviceToHost, stream));
    return h;
  };
  const std::vector<uint32_t> fr_row = down_u32(F.r_row, (size_t)F.nc + 1), fr_col = down_u32(F.r_col, F.n);
  const std::vector<uint32_t> mr_row = down_u32(M.r_row, (size_t)nc + 1), mr_col = down_u32(M.r_col, nm);
  std::vector<uint32_t> mrow, mcsr;  // the off-diagonal pattern of level i + 1
  if (!level_csr(M, mrow, mcsr) || F.nc != nm) return false;
  // 256-thread blocks (one CU each, like the k_amg_resrestrict launches they
  // replace) while the ring's redundant level-i rows stay within 50 %
  // (profiles/r06/ab_log.md, C1: levels 4+5 at 1.41x rows 7.8 us against
  // 5.5 + 5.1; levels 2+3 at 2.9x 16.1 us against 7.1 + 6.3; 1,024-thread
  // blocks -- less redundancy, a quarter of the CUs -- lost on both pairs)
  PairPartition pp;
  const uint32_t threads = 256;
  if (!build_pair_partition(fr_row, fr_col, mr_row, mr_col, mrow, mcsr, threads, pp)) return false;
  if (pair_mode < 2 && (double)pp.f.size() > 1.5 * (double)F.n) return false;
  const std::vector<uint16_t> lc = to_slots(M, mrow, pp.lc);
  AmgPairImage& P = rr_pair[i];
  P.nblocks = (uint32_t)pp.jb.size() - 1;
  P.threads = threads;
  P.jb = arena.upload(pp.jb, stream);
  P.sb = arena.upload(pp.sb, stream);
  P.s = arena.upload(pp.s, stream);
  P.fo = arena.upload(pp.fo, stream);
  P.f = arena.upload(pp.f, stream);
  P.lc = arena.upload(lc, stream);
  sync();
  return true;
}

// LDS image of the tail levels [tf, L) for k_amg_tail_blob: every array the
// tail V-cycle reads, compacted (off-diagonal CSR, u16 indices) from the
// level images, when vectors + blob fit in one CU's LDS.
void Solver::build_tail_blob(int tf, bool reuse) {
  const uint32_t old_words = tail_blob_words;
  tail_blob_first = -1;
  const int L = (int)levels.size();
  if (tf >= L) return;
  std::vector<uint32_t> blob;
  std::vector<TailBlobLevel> desc(L);
  auto align4 = [&] {
    while (blob.size() % 4) blob.push_back(0);
    return (uint32_t)blob.size();
  };
  auto put_f = [&](const float* v, size_t n) {
    const uint32_t o = align4();
    for (size_t i = 0; i < n; ++i) {
      uint32_t w;
      std::memcpy(&w, v + i, 4);
      blob.push_back(w);
    }
    return o;
  };
  auto put_u32 = [&](const std::vector<uint32_t>& v) {
    const uint32_t o = align4();
    blob.insert(blob.end(), v.begin(), v.end());
    return o;
  };
  auto put_u16 = [&](const std::vector<uint32_t>& v) {
    const uint32_t o = align4();
    for (size_t i = 0; i < v.size(); i += 2)
      blob.push_back((v[i] & 0xFFFFu) | ((i + 1 < v.size() ? v[i + 1] & 0xFFFFu : 0u) << 16));
    return o;
  };
  auto put_u8 = [&](const std::vector<uint8_t>& v) {
    const uint32_t o = align4();
    for (size_t i = 0; i < v.size(); i += 4) {
      uint32_t w = 0;
      for (size_t b = 0; b < 4 && i + b < v.size(); ++b) w |= (uint32_t)v[i + b] << (8 * b);
      blob.push_back(w);
    }
    return o;
  };
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) CFD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
  };
  uint32_t vec = 0;
  for (int l = tf; l < L; ++l) {
    const AmgLevelDev& d = levels[l].dev;
    const uint32_t n = d.n;
    if (n > 65535 || d.nc > 65535 || levels[l].wide) return;  // the blob keeps u8 diagonal ranks
    std::vector<uint8_t> drank(n);
    std::vector<float> dv(n), de(n), vals;
    d2h(drank.data(), d.drank, n);
    d2h(dv.data(), d.dv, (size_t)n * 4);
    d2h(de.data(), d.de, (size_t)n * 4);
    std::vector<uint32_t> agg, rrow, rcol, ro, cols;
    if (d.nc) {
      agg.resize(n);
      rrow.resize((size_t)d.nc + 1);
      d2h(agg.data(), d.agg, (size_t)n * 4);
      d2h(rrow.data(), d.r_row, rrow.size() * 4);
    }
    if (!level_csr(d, ro, cols, &vals)) return;  // tail levels are replicated: global columns
    if (d.nc) {
      rcol.resize(rrow[d.nc]);
      d2h(rcol.data(), d.r_col, rcol.size() * 4);
      sync();
    }
    TailBlobLevel& D = desc[l];
    D.n = n;
    D.nc = d.nc;
    D.maxlen = 0;
    for (uint32_t i = 0; i < n; ++i) D.maxlen = std::max(D.maxlen, ro[i + 1] - ro[i]);
    D.de = put_f(de.data(), n);
    D.dv = put_f(dv.data(), n);
    D.rowoff = put_u32(ro);
    D.drank = put_u8(drank);
    D.val = put_f(vals.data(), vals.size());
    D.col = put_u16(cols);
    if (d.nc) {
      D.agg = put_u16(agg);
      D.r_row = put_u16(rrow);
      D.r_col = put_u16(rcol);
    }
    vec += 4 * ((n + 3) & ~3u);
  }
  align4();
  if (4 * ((size_t)vec + blob.size()) > lds_budget) return;
  if (reuse && d_tail_blob && blob.size() == old_words) {  // same structure: new values in place
    CFD_HIP(hipMemcpyAsync(d_tail_blob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, stream));
    CFD_HIP(hipMemcpyAsync(d_tail_desc, desc.data(), desc.size() * sizeof(TailBlobLevel), hipMemcpyHostToDevice,
                           stream));
    sync();  // the host staging vectors die here
  } else {
    if (reuse) throw std::logic_error("AMG refresh: tail blob layout changed");
    d_tail_blob = arena.upload(blob, stream);
    d_tail_desc = arena.upload(desc, stream);
  }
  tail_blob_words = (uint32_t)blob.size();
  tail_vec_floats = vec;
  tail_blob_first = tf;
}

// Timing of level-0 smoother launches (bench roofline): a pair of pool events
// per launch, recorded by the GPU at kernel start / end (hipExtLaunchKernel).
// The pool is created before the timed steps (cfd_profile_reset) and grows
// without synchronising; only at kProfPoolMax events is it drained (a stream
// synchronisation) into prof_ms.
std::pair<hipEvent_t, hipEvent_t> Solver::prof_pair() {
  if (prof_used + 2 > prof_ev.size()) {
    if (prof_ev.size() < kProfPoolMax) {
      prof_grow(prof_ev.size() + 1024);  // no synchronisation inside the timed steps
    } else {
      CFD_HIP(hipStreamSynchronize(stream));
      for (size_t k = 0; k + 1 < prof_used; k += 2) {
        float ms = 0.0f;
        CFD_HIP(hipEventElapsedTime(&ms, prof_ev[k], prof_ev[k + 1]));
        prof_ms += ms;
      }
      prof_used = 0;
    }
  }
  prof_used += 2;
  return {prof_ev[prof_used - 2], prof_ev[prof_used - 1]};
}

void Solver::prof_grow(size_t n) {
  while (prof_ev.size() < n) {
    hipEvent_t e;
    CFD_HIP(hipEventCreate(&e));
    prof_ev.push_back(e);
  }
}

void Solver::amg_smooth(size_t li, float*& xcur, const float* b, bool x_zero, bool nt) {
  AmgGpuLevel& L = levels[li];
  if (x_zero) {
    launch_amg_smooth_zero(L.dev, b, L.xt, stream);
  } else if (li == 0 && prof_take()) {
    if (capturing) {  // event nodes of the graph around the launch, read per replay (graph_harvest)
      hipEvent_t e0, e1;
      CFD_HIP(hipEventCreate(&e0));
      capturing->ev.push_back(e0);
      CFD_HIP(hipEventCreate(&e1));
      capturing->ev.push_back(e1);
      CFD_HIP(hipEventRecordWithFlags(e0, stream, hipEventRecordExternal));
      launch_amg_smooth(L.dev, xcur, b, L.xt, stream, nullptr, nullptr, nt);
      CFD_HIP(hipEventRecordWithFlags(e1, stream, hipEventRecordExternal));
    } else {
      const auto ev = prof_pair();
      launch_amg_smooth(L.dev, xcur, b, L.xt, stream, ev.first, ev.second, nt);
      prof_launches++;
    }
  } else {
    launch_amg_smooth(L.dev, xcur, b, L.xt, stream, nullptr, nullptr, nt);
  }
  std::swap(xcur, L.xt);  // out-of-place Jacobi: the partner buffer becomes current
}

// amg.rs:666-770, level 0 bound to (x = p_sol, b = temp_p): runs the schedule
// the setup planned (vc_plan).  Which launches there are is the plan's; how a
// row-partitioned level (below amg_g on a distributed rank) runs one is
// decided here: each smoother input gets a halo (the cleared coarse x needs
// none), the restriction and the prolongation split around their exchange.
void Solver::v_cycle() {
  const int L = (int)levels.size();
  levels[0].x = p_sol;
  levels[0].b = temp_p;
  if (ref_inplace || ref_clamp) {
    v_cycle_reference();
    return;
  }
  if (vc_plan.empty()) throw std::logic_error("AMG V-cycle without a schedule");
  // smoother sweep; on a distributed level the x halo overlaps the interior rows
  // post: the up-sweep's smoother (nontemporal matrix loads with nt_mask bit 1)
  auto sm = [&](int i, bool x_zero, bool post = false) {
    AmgGpuLevel& Lv = levels[i];
    const bool ntl = nt(post ? 1u : 16u);
    if (!Lv.dist || x_zero) {
      amg_smooth(i, Lv.x, Lv.b, x_zero, ntl);
      return;
    }
    const bool timed = i == 0 && prof_take();  // kernel time only: each part timed separately
    const CommScope cs(this, amg_cat(i));
    overlapped(Lv.plan, {{Lv.x, 1}}, Lv.dev.n, [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
      const auto ev = timed ? prof_pair() : std::pair<hipEvent_t, hipEvent_t>{};  // untimed: no events
      launch_amg_smooth(with_rows(Lv.dev, a, b, a2, b2), Lv.x, Lv.b, Lv.xt, stream, ev.first, ev.second, ntl);
    });
    if (timed) prof_launches++;
    std::swap(Lv.x, Lv.xt);
  };
  auto res = [&](int i) {
    AmgGpuLevel& Lv = levels[i];
    auto f = [&](uint32_t a, uint32_t b, uint32_t a2, uint32_t b2) {
      launch_amg_residual(with_rows(Lv.dev, a, b, a2, b2), Lv.x, Lv.b, Lv.r, stream,
                          (i == 0 && nt(2)) || (i == 1 && nt(64)));
    };
    if (Lv.dist) {
      const CommScope cs(this, amg_cat(i));
      overlapped(Lv.plan, {{Lv.x, 1}}, Lv.dev.n, f);
    } else {
      f(0, Lv.dev.n, 0, 0);
    }
  };
  // restriction of level i's residual; smo: the coarse level's zero-x sweep fused in
  auto restrict_r = [&](int i, float* smo) {
    AmgGpuLevel &Lv = levels[i], &C = levels[i + 1];
    if (!Lv.dist) {
      launch_amg_restrict(Lv.dev, Lv.r, C.b, C.x, 0, 0, 0, stream, smo, C.dev.de);
      return;
    }
    // the restriction sums members owned by the next ranks too (their residuals
    // are ghosts): the aggregates without such members overlap the exchange
    const bool into_dist = C.dist;
    float* cb = into_dist ? C.b : C.b + C.C0;
    float* cx = into_dist ? C.x : C.x + C.C0;
    const uint32_t sc = into_dist ? C.npad : Lv.dev.nc;
    const uint32_t cg_lo = into_dist ? C.glo : (uint32_t)C.C0;
    const uint32_t cg_hi = into_dist ? C.ghi : (uint32_t)(C.nglob - C.C1);
    if (amg_local) {  // partition-aware: every member is owned, no residual halo
      launch_amg_restrict(Lv.dev, Lv.r, cb, cx, sc, cg_lo, cg_hi, stream, smo, C.dev.de, 0, Lv.dev.nc, true);
    } else {
      const uint32_t split = Lv.dev.n >= overlap_min_rows ? Lv.rc_hi : 0u;  // as overlapped()
      const CommScope cs(this, amg_cat(i));
      halo_begin(Lv.plan, {{Lv.r, 1}});
      if (split > 0)
        launch_amg_restrict(Lv.dev, Lv.r, cb, cx, sc, cg_lo, cg_hi, stream, smo, C.dev.de, 0, split, false);
      halo_end();
      launch_amg_restrict(Lv.dev, Lv.r, cb, cx, sc, cg_lo, cg_hi, stream, smo, C.dev.de, split, Lv.dev.nc, true);
    }
  };
  // x_i += P x_{i+1}; a row-partitioned coarse level: the prolongation reads
  // aggregates seeded on lower ranks (ghosts of the coarse x)
  auto prolong = [&](int i) {
    AmgGpuLevel &F = levels[i], &C = levels[i + 1];
    if (C.dist && amg_local) {  // partition-aware: every fine row's aggregate is owned
      launch_amg_prolong(F.dev, F.x, C.x, stream, 0, F.dev.n, nt(32));
    } else if (C.dist) {  // the rows of owned aggregates overlap the coarse-x exchange
      const uint32_t split = F.dev.n >= overlap_min_rows ? F.pf_lo : F.dev.n;  // as overlapped()
      const CommScope cs(this, amg_cat(i + 1));
      halo_begin(C.plan, {{C.x, 1}});
      if (split < F.dev.n) launch_amg_prolong(F.dev, F.x, C.x, stream, split, F.dev.n, nt(32));
      halo_end();
      if (split > 0) launch_amg_prolong(F.dev, F.x, C.x, stream, 0, split, nt(32));
    } else {
      launch_amg_prolong(F.dev, F.x, C.x, stream, 0, 0, nt(32));
    }
  };
  for (const VcOp& op : vc_plan) {
    const int i = op.level;
    AmgGpuLevel& Lv = levels[i];
    switch (op.kind) {
      case VcKind::PreSmooth: sm(i, op.flag); break;
      case VcKind::TakePreSmoothed: std::swap(Lv.x, Lv.xt); break;
      case VcKind::ResRestrictFused: {
        AmgGpuLevel& C = levels[i + 1];
        launch_amg_resrestrict(Lv.dev, Lv.x, Lv.b, C.b, C.x, op.flag ? C.xt : nullptr, C.dev.de, stream);
        break;
      }
      case VcKind::ResidualRestrict:
        res(i);
        restrict_r(i, op.flag ? levels[i + 1].xt : nullptr);
        break;
      case VcKind::ResRestrictPair: {
        // level i + 1 ends pre-smoothed (as a TakePreSmoothed would leave it)
        // and level i + 2 gets its rhs
        AmgGpuLevel &C = levels[i + 1], &C2 = levels[i + 2];
        launch_amg_resrestrict_pair(Lv.dev, C.dev, rr_pair[i], Lv.x, Lv.b, C.b, C.xt, C2.b, C2.x,
                                    op.flag ? C2.xt : nullptr, C2.dev.de, stream);
        std::swap(C.x, C.xt);
        break;
      }
      case VcKind::GatherRhs: {  // level i - 1 restricted into its own slice
        std::vector<size_t> off(R + 1);
        for (int q = 0; q <= R; ++q) off[q] = Lv.part[q] * sizeof(float);
        timed_gather(kCommRepGather, off[rk + 1] - off[rk], [&] { comm->allgatherv_inplace(Lv.b, off, stream); });
        break;
      }
      case VcKind::TailBlob:
        launch_amg_tail_blob(d_tail, d_tail_desc, d_tail_blob, tail_blob_words, tail_vec_floats, i, L, Lv.b, Lv.dev.n,
                             stream);
        break;
      case VcKind::Tail: {
        size_t lds = 0;  // LDS-resident tail when its vectors fit (CFD_AMG_TAIL=global: never)
        for (int l = i; l < L; ++l) lds += 4 * (((size_t)levels[l].dev.n + 3) & ~(size_t)3) * sizeof(float);
        if (lds > lds_budget || tail_form == 0) lds = 0;
        launch_amg_tail(d_tail, i, L, lds, stream);
        break;
      }
      case VcKind::CoarsestSweeps:
        for (int s = 0; s < 10; ++s) sm(i, s == 0 && i > 0);
        break;
      case VcKind::Prolong: prolong(i); break;
      case VcKind::PostSmooth: sm(i, false, true); break;
      case VcKind::PostSmoothProlong:
        // the prolongation applied inside the post-smoother's reads (x stays un-prolonged)
        launch_amg_smooth_prolong(Lv.dev, Lv.x, levels[i + 1].x, Lv.b, Lv.xt, stream);
        std::swap(Lv.x, Lv.xt);
        break;
      case VcKind::ProlongSmoothPair: {
        // level i's smoothed x lives only in the kernel's LDS (nothing reads it
        // after the up-leg), its buffers swap as the separate launch would leave them
        AmgGpuLevel& F = levels[i - 1];
        launch_amg_prolong_smooth_pair(F.dev, Lv.dev, up_pair[i], F.x, F.b, F.xt, Lv.x, Lv.b, levels[i + 1].x, stream);
        std::swap(Lv.x, Lv.xt);
        std::swap(F.x, F.xt);
        break;
      }
    }
  }
  // every level performs an even number of sweeps, so level 0 ends in p_sol
  if (levels[0].x != p_sol) throw std::logic_error("AMG level-0 ping-pong parity");
}

// amg.rs:666-770 dispatch by dispatch (test mode, flags 1 / 8): pre-smooth,
// residual + restriction (+ the clamped rows' store onto the last coarse
// entry), the coarse x cleared, 10 coarsest sweeps, prolongation +
// post-smooth -- no fused forms, no tail kernel.  In place (flag 1) the
// smoother runs its workgroups in order; else out-of-place Jacobi.
void Solver::v_cycle_reference() {
  const int L = (int)levels.size();
  auto smooth = [&](int i) {
    AmgGpuLevel& Lv = levels[i];
    if (ref_inplace) {
      launch_amg_smooth_ordered(Lv.dev, Lv.x, Lv.b, stream);
    } else {
      launch_amg_smooth(Lv.dev, Lv.x, Lv.b, Lv.xt, stream);
      std::swap(Lv.x, Lv.xt);
    }
  };
  for (int i = 0; i + 1 < L; ++i) {
    AmgGpuLevel &F = levels[i], &C = levels[i + 1];
    smooth(i);
    launch_amg_residual(F.dev, F.x, F.b, F.r, stream);
    launch_amg_restrict(F.dev, F.r, C.b, C.x, 0, 0, 0, stream);  // coarse b = R r, coarse x = 0
    const uint32_t nc = C.dev.n;
    if (ref_clamp && nc % 64 != 0) CFD_HIP(hipMemsetAsync(C.b + nc - 1, 0, sizeof(float), stream));
  }
  for (int s = 0; s < 10; ++s) smooth(L - 1);
  for (int i = L - 2; i >= 0; --i) {
    launch_amg_prolong(levels[i].dev, levels[i].x, levels[i + 1].x, stream);
    smooth(i);
  }
  if (levels[0].x != p_sol) throw std::logic_error("AMG level-0 ping-pong parity (reference semantics)");
}

}  // namespace cfd2
