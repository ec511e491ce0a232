// Host driver of the HIP coupled step: restates the control flow of
//   coupled_solver.rs:33-580            step_coupled / check_evolution
//   coupled_solver_fgmres.rs:1728-2448  solve_coupled_fgmres (FGMRES(50) + Schur)
//   linear_solver/amg.rs:666-770        v_cycle (amg_cycle.cpp)
//   solver.rs:9-44, 97-128, 276-294     set_u / set_p / set_dt / getters / history
// over the kernels of ../hip/*.hip, on one HIP stream.  All vectors stay
// in HBM; host round trips are the ones the reference control flow needs
// (blocking norms at solve start / restart, lagged residual reads), and none
// under the fixed benchmark schedule except the two early-exit norms.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <cstring>
#include <limits>

#include "solver_impl.hpp"

namespace cfd2 {

namespace {
// Rust's `{:.2e}` (the reference's log format): 1.23e-5, 3.40e38, NaN, inf
std::string e2(double v) {
  if (std::isnan(v)) return "NaN";
  if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[48];
  std::snprintf(buf, sizeof(buf), "%.2e", v);
  const std::string s(buf);
  const size_t e = s.find('e');
  size_t i = e + 1;
  const bool neg = s[i] == '-';
  if (s[i] == '-' || s[i] == '+') ++i;
  while (i + 1 < s.size() && s[i] == '0') ++i;
  return s.substr(0, e) + "e" + (neg ? "-" : "") + s.substr(i);
}
const char* tf(bool b) { return b ? "true" : "false"; }
// device scalars dsc[0..15]: rhs_norm, resid, inv_resid, wnorm, inv_w, resid_est
constexpr int kHOff = 16;
}  // namespace

template <class T>
T* Solver::valloc(int comps) {
  T* base = arena.alloc<T>(vlen * comps + 64);
  CFD_HIP(hipMemsetAsync(base, 0, (vlen * comps + 64) * sizeof(T), stream));
  return base + (size_t)shift * comps;
}

void Solver::make_plan_buffers(HaloPlan& p, int max_comps) {
  p.d_send_idx = arena.upload(p.send_idx, stream);
  p.max_comps = max_comps;
  p.d_stage = arena.alloc<float>(p.send_idx.size() * (size_t)max_comps + 1);
}

Solver::Solver(const cfd_mesh_view& mesh, const cfd_config& c, int dev, std::unique_ptr<Comm> cm)
    : cfg(c), device(dev) {
  if (cfg.max_restart < 1 || cfg.max_restart > 63) throw std::invalid_argument("max_restart must be 1..63");
  m = cfg.max_restart;
  m1 = m + 1;
  NG = mesh.num_cells;
  if (cm && cm->size > 1) {
    comm = std::move(cm);
    R = comm->size;
    rk = comm->rank;
  }
  starts = partition_starts(NG, R);
  build_topology(mesh, topo, (uint32_t)starts[rk], (uint32_t)starts[rk + 1]);
  N = topo.N;
  F = topo.F;
  // flow diagnostics (diagnostics.cpp): the host data the mesh view is needed for
  min_cell = std::numeric_limits<double>::infinity();
  for (uint32_t i = 0; i < NG; ++i) min_cell = std::fmin(min_cell, std::sqrt(mesh.cell_vol[i]));
  for (uint32_t i = 0; i < NG; ++i)
    for (uint32_t k = mesh.cell_face_offsets[i]; k < mesh.cell_face_offsets[i + 1]; ++k) {
      const uint32_t f = mesh.cell_faces[k];
      if (f >= mesh.num_faces) throw std::invalid_argument("cell_faces out of range");
      if (mesh.face_neighbor[f] == UINT32_MAX && (mesh.face_boundary[f] & 3u) == 3u)
        wall_faces.push_back({mesh.face_cx[f], mesh.face_cy[f], i, k - mesh.cell_face_offsets[i]});
    }
  red = red_geom(NG);
  if (red.nseg > kRedMaxSegments)
    throw std::invalid_argument("mesh too large for the reduction tree (at most 268 M cells)");
  nchunks = (N + kRedChunkCells - 1) / kRedChunkCells;
  nunits = (nchunks + red.U - 1) / red.U;
  pstride = (nunits + 3) & ~3u;
  shift = (topo.glo + 63) & ~63u;
  vlen = (size_t)shift + topo.npad + topo.ghi;
  CFD_HIP(hipSetDevice(device));
  lds_budget = init_kernel_attributes(device);
  amg_wide_limit = (int)std::max<uint64_t>(1, std::min<uint64_t>(255, knob_u64(Knob::AmgWideLimit, 255)));
  check_sync = cfg.log_level >= 3;  // debug: synchronise and check after every launch
  small_forms = knob_on(Knob::SmallMeshForms);
  nt_mask = (unsigned)knob_u64(Knob::Nt, nt_mask);
  // C1-size meshes: 64 MB of the dots pass kept in the Infinity Cache for a
  // top-down update (profiles/r04/ab_cgskeep2_c1.txt: update 36.5-36.9 ->
  // 32.3 us, dots +0.3 us per iteration); from 2^22 cells on the kept lines
  // cost more than they return (ab_cgskeep_c2.txt: dots 284 -> 293 us)
  cgs_keep_bytes = !cgs_serial_form(N) ? (size_t)64 << 20 : 0;
  CFD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  amg_local = dist() && cfg.amg_local_aggregation != 0;
  // hipGraph replay: opt-in through cfd_graph_enable (replay measured no faster
  // than eager launches on this pool, profiles/r05/ab_graph_c0_c1.txt: C0
  // 13.36-13.47 vs 13.30-13.51 ms/step, C1 39.6-39.9 vs 38.8-39.1); halo
  // exchanges and collectives stay eager
  graph_on = false;
  if (dist()) {
    overlap_min_rows = (uint32_t)knob_u64(Knob::OverlapMinRows, overlap_min_rows);
    CFD_HIP(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
    CFD_HIP(hipEventCreateWithFlags(&hev_pack, hipEventDisableTiming));
    CFD_HIP(hipEventCreateWithFlags(&hev_done, hipEventDisableTiming));
    cell_plan = build_halo_plan(starts, rk, topo.srow.data(), N, topo.scol.data(), topo.ghost, topo.glo,
                                topo.npad);
    make_plan_buffers(cell_plan, 8);
    // segments of every rank (ranks own whole segments: partition_starts)
    std::vector<uint32_t> src(red.nseg);
    for (int q = 0; q < R; ++q) {
      const uint64_t s0 = starts[q] / red.seg_cells;
      const uint64_t s1 = (starts[q + 1] + red.seg_cells - 1) / red.seg_cells;
      maxseg = std::max(maxseg, (uint32_t)(s1 - s0));
      for (uint64_t sg = s0; sg < s1; ++sg) src[sg] = ((uint32_t)q << 20) | (uint32_t)(sg - s0);
    }
    if (maxseg >= (1u << 20) || R >= (1 << 12)) throw std::invalid_argument("too many segments / ranks");
    d_seg_src = arena.upload(src, stream);
    red_local = arena.alloc<float>((size_t)m1 * maxseg);
    red_gather = arena.alloc<float>((size_t)R * m1 * maxseg);
    red_local_d = arena.alloc<double>((size_t)5 * maxseg);
    red_gather_d = arena.alloc<double>((size_t)R * 5 * maxseg);
    mx_gather = arena.alloc<uint32_t>(2 * (size_t)R);
    d_u64 = arena.alloc<uint64_t>((size_t)R + 1);  // not lazily: the AMG build runs on amg_arena
    // check_evolution's stride bug reads records (i >> 2) of the global state
    ev_a = (uint64_t)topo.c0 >> 2;
    ev_b = (((uint64_t)topo.c1 - 1) >> 2) + 1;
    const size_t ne = ev_b - ev_a;
    evrec.u = arena.alloc<float2>(ne);
    evrec.p = arena.alloc<float>(ne);
    evrec.dp = arena.alloc<float>(ne);
    evrec.gp = arena.alloc<float2>(ne);
  }
  // static mesh data
  d_vol = arena.upload(topo.vol, stream);
  fs.other = arena.upload(topo.fs_other, stream);
  fs.meta = arena.upload(topo.fs_meta, stream);
  fs.area = arena.upload(topo.fs_area, stream);
  fs.nx = arena.upload(topo.fs_nx, stream);
  fs.ny = arena.upload(topo.fs_ny, stream);
  fs.lam_s = arena.upload(topo.fs_lam_s, stream);
  fs.lam_f = arena.upload(topo.fs_lam_f, stream);
  fs.dist_a = arena.upload(topo.fs_dist_a, stream);
  fs.dist_e = arena.upload(topo.fs_dist_e, stream);
  fs.dvx = arena.upload(topo.fs_dvx, stream);
  fs.dvy = arena.upload(topo.fs_dvy, stream);
  fs.rx = arena.upload(topo.fs_rx, stream);
  fs.ry = arena.upload(topo.fs_ry, stream);
  fs.rox = arena.upload(topo.fs_rox, stream);
  fs.roy = arena.upload(topo.fs_roy, stream);
  fs.nface = arena.upload(topo.nface, stream);
  fs.wf = topo.wf;
  d_scol = arena.upload(topo.ell_col, stream);
  d_slen = arena.upload(topo.ell_len, stream);
  d_sdrank = arena.upload(topo.ell_drank, stream);
  if (topo.use16) d_scol16 = arena.upload(topo.ell_col16, stream);
  d_slen8 = arena.upload(topo.ell_len8, stream);
  d_sdrank8 = arena.upload(topo.ell_drank8, stream);
  if (topo.use16)
    d_tcol16 = arena.upload(topo.tcol16, stream);
  else
    d_tcol = arena.upload(topo.tcol, stream);
  d_tlg = arena.upload(topo.tlg, stream);
  d_tdrank8 = arena.upload(topo.tdrank8, stream);
  // fields (init/fields.rs:62-139): zero-initialised, with ghost space
  auto zeros_state = [&](StateView& v) {
    v.u = valloc<float2>(1);
    v.p = valloc<float>(1);
    v.dp = valloc<float>(1);
    v.gp = valloc<float2>(1);
  };
  for (auto& r : ring) zeros_state(r);
  zeros_state(prev);
  dp_scratch = valloc<float>(1);
  gp_scratch = valloc<float2>(1);
  const size_t slots_f = (size_t)topo.wf * N, slots_s = (size_t)topo.ws * topo.ld;
  flux_s = arena.alloc<float>(slots_f);
  CFD_HIP(hipMemsetAsync(flux_s, 0, slots_f * sizeof(float), stream));
  grad_u = valloc<float2>(1);
  grad_v = valloc<float2>(1);
  cval_a = arena.alloc<float2>(slots_s);
  cval_g = arena.alloc<float2>(slots_s);
  CFD_HIP(hipMemsetAsync(cval_a, 0, slots_s * sizeof(float2), stream));
  CFD_HIP(hipMemsetAsync(cval_g, 0, slots_s * sizeof(float2), stream));
  cdiag2 = arena.alloc<float2>(topo.ld);
  CFD_HIP(hipMemsetAsync(cdiag2, 0, topo.ld * sizeof(float2), stream));
  sval = arena.alloc<float>(slots_s);
  CFD_HIP(hipMemsetAsync(sval, 0, slots_s * sizeof(float), stream));
  rhs = valloc<float>(3);
  x = valloc<float>(3);
  dinv_uv = valloc<float>(1);
  dinv_p = valloc<float>(1);
  partial_d = arena.alloc<double>(5 * (size_t)pstride + 5);
  maxbits = arena.alloc<uint32_t>(4);
  blockmax = arena.alloc<uint32_t>(2 * (((size_t)N + 255) / 256) + 2);
  // pinned, mapped (for every device: portable) and coherent: kernels may store
  // the per-iteration residual into it directly (d_pin, the device view),
  // visible to the host after the event
  CFD_HIP(hipHostMalloc((void**)&h_pin, 4096 * sizeof(float),
                        hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable));
  CFD_HIP(hipHostGetDevicePointer((void**)&d_pin, h_pin, 0));
  for (auto& e : ev_outer) CFD_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // constants (init/fields.rs:100-115)
  constants.dt = 0.0001f;
  constants.dt_old = 0.0001f;
  constants.time = 0.0f;
  constants.viscosity = 0.01f;
  constants.density = 1.0f;
  constants.component = 0;
  constants.alpha_p = 1.0f;
  constants.scheme = 0;
  constants.alpha_u = 0.7f;
  constants.stride_x = 65535u * 64u;
  constants.time_scheme = 0;
  constants.inlet_velocity = 1.0f;
  constants.ramp_time = 0.1f;
  constants.precond_type = 0;
  std::memset(&info, 0, sizeof(info));
  sync();
}

Solver::~Solver() {
  if (stream) (void)hipStreamSynchronize(stream);
  for (IterGraph& G : graphs) {
    if (G.exec) (void)hipGraphExecDestroy(G.exec);
    for (auto e : G.ev) (void)hipEventDestroy(e);
  }
  for (auto e : ev_iter) (void)hipEventDestroy(e);
  for (auto e : ev_outer)
    if (e) (void)hipEventDestroy(e);
  for (auto e : prof_ev) (void)hipEventDestroy(e);
  if (cstream) (void)hipStreamSynchronize(cstream);
  for (auto e : comm_ev_pool) (void)hipEventDestroy(e);
  if (h_pin) (void)hipHostFree(h_pin);
  if (cstream) (void)hipStreamSynchronize(cstream);
  if (hev_pack) (void)hipEventDestroy(hev_pack);
  if (hev_done) (void)hipEventDestroy(hev_done);
  comm.reset();
  arena.release();
  amg_arena.release();
  sc_arena.release();
  if (cstream) (void)hipStreamDestroy(cstream);
  if (stream) (void)hipStreamDestroy(stream);
}

CoupledMatrix Solver::cmat() const {
  CoupledMatrix A;
  A.N = N;
  A.r0 = 0;
  A.r1 = N;
  A.r2 = A.r3 = 0;
  A.ld = topo.ld;
  A.ws = topo.ws;
  A.use16 = topo.use16 ? 1 : 0;
  A.col = d_tcol;
  A.col16 = d_tcol16;
  A.lg = d_tlg;
  A.drank = d_tdrank8;
  A.cval_a = cval_a;
  A.cval_g = cval_g;
  A.cdiag2 = cdiag2;
  A.reg = !topo.tmode.empty() && topo.ws <= kCoupledRegMaxWs ? 1 : 0;
  for (int r = 0; r < 8; ++r) A.tmode[r] = r < (int)topo.tmode.size() ? topo.tmode[r] : 0;
  return A;
}

void Solver::log(const char* fmt, ...) const {
  if (cfg.log_level < 1 || rk != 0) return;
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------- state API
// set_u / set_p take the GLOBAL per-cell arrays; a distributed rank keeps its
// owned cells and ghosts.  Getters return the owned cells.
void Solver::set_u(const double* uv) {  // solver.rs:9-21 (clobbers the whole state)
  CFD_HIP(hipSetDevice(device));
  std::vector<float> img;
  local_image(uv, 2, img);
  StateView& s = S();
  CFD_HIP(hipMemcpyAsync(vbase(s.u, 1), img.data(), vlen * sizeof(float2), hipMemcpyHostToDevice, stream));
  CFD_HIP(hipMemsetAsync(vbase(s.p, 1), 0, vlen * sizeof(float), stream));
  CFD_HIP(hipMemsetAsync(vbase(s.dp, 1), 0, vlen * sizeof(float), stream));
  CFD_HIP(hipMemsetAsync(vbase(s.gp, 1), 0, vlen * sizeof(float2), stream));
  sync();
}

void Solver::set_p(const double* pv) {  // solver.rs:23-34
  CFD_HIP(hipSetDevice(device));
  std::vector<float> img;
  local_image(pv, 1, img);
  StateView& s = S();
  CFD_HIP(hipMemsetAsync(vbase(s.u, 1), 0, vlen * sizeof(float2), stream));
  CFD_HIP(hipMemcpyAsync(vbase(s.p, 1), img.data(), vlen * sizeof(float), hipMemcpyHostToDevice, stream));
  CFD_HIP(hipMemsetAsync(vbase(s.dp, 1), 0, vlen * sizeof(float), stream));
  CFD_HIP(hipMemsetAsync(vbase(s.gp, 1), 0, vlen * sizeof(float2), stream));
  sync();
}

namespace {
void copy_state(const StateView& src, StateView& dst, size_t off, size_t n, hipStream_t s) {
  CFD_HIP(hipMemcpyAsync(dst.u - off, src.u - off, n * sizeof(float2), hipMemcpyDeviceToDevice, s));
  CFD_HIP(hipMemcpyAsync(dst.p - off, src.p - off, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  CFD_HIP(hipMemcpyAsync(dst.dp - off, src.dp - off, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  CFD_HIP(hipMemcpyAsync(dst.gp - off, src.gp - off, n * sizeof(float2), hipMemcpyDeviceToDevice, s));
}
}  // namespace

void Solver::initialize_history() {  // solver.rs:276-294
  CFD_HIP(hipSetDevice(device));
  copy_state(ring[i_state], ring[i_old], shift, vlen, stream);
  copy_state(ring[i_state], ring[i_old_old], shift, vlen, stream);
  sync();
}

void Solver::get_u(double* uv) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float2> u(N);
  CFD_HIP(hipMemcpyAsync(u.data(), S().u, N * sizeof(float2), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) {
    uv[2 * i] = u[i].x;
    uv[2 * i + 1] = u[i].y;
  }
}

void Solver::get_p(double* out) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float> p(N);
  CFD_HIP(hipMemcpyAsync(p.data(), S().p, N * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) out[i] = p[i];
}

void Solver::get_d_p(double* out) {
  CFD_HIP(hipSetDevice(device));
  std::vector<float> p(N);
  CFD_HIP(hipMemcpyAsync(p.data(), S().dp, N * sizeof(float), hipMemcpyDeviceToHost, stream));
  sync();
  for (uint32_t i = 0; i < N; ++i) out[i] = p[i];
}

// ------------------------------------------------------------ distribution
// Halo exchange of per-cell fields over `plan`: pack the rows the peers need,
// then one grouped transfer per (peer, field) straight into the ghost slots.
void Solver::halo(HaloPlan& plan, std::initializer_list<HField> fields) {
  if (!dist()) return;
  halo_begin(plan, fields);
  halo_end();
}

void Solver::halo_end() {
  if (!comm_prof) {
    CFD_HIP(hipStreamWaitEvent(stream, hev_done, 0));
    return;
  }
  // the compute stream's stall on the exchange: from reaching the wait to its release
  hipEvent_t a = comm_event(), b = comm_event();
  CFD_HIP(hipEventRecord(a, stream));
  CFD_HIP(hipStreamWaitEvent(stream, hev_done, 0));
  CFD_HIP(hipEventRecord(b, stream));
  comm_recs.push_back({halo_cat, 0, a, b});
}

// The pool grows for as long as comm_prof is on: a drain (both streams
// synchronised) inside the timed step would stall it and shift the waits
// measured after it (a C4 step records ~18 k events).  The pool
// is folded and reused only by comm_drain() (cfd_comm_timing, enable/disable).
hipEvent_t Solver::comm_event() {
  if (comm_ev_used == comm_ev_pool.size()) {
    for (int k = 0; k < 1024; ++k) {
      hipEvent_t e;
      CFD_HIP(hipEventCreate(&e));
      comm_ev_pool.push_back(e);
    }
  }
  return comm_ev_pool[comm_ev_used++];
}

void Solver::comm_drain() {
  if (comm_recs.empty()) return;
  CFD_HIP(hipStreamSynchronize(stream));
  if (cstream) CFD_HIP(hipStreamSynchronize(cstream));
  for (const CommRec& r : comm_recs) {
    float ms = 0.0f;
    CFD_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    CommTimes& t = comm_times[r.cat];
    if (r.kind == 0 || r.kind == 2) t.wait_ms += ms;
    if (r.kind == 1 || r.kind == 2) t.comm_ms += ms;
  }
  comm_recs.clear();
  comm_ev_used = 0;
}

void Solver::comm_prof_reset() {
  comm_drain();
  for (CommTimes& t : comm_times) t = CommTimes{};
}

void Solver::halo_begin(HaloPlan& plan, std::initializer_list<HField> fields) {
  const uint32_t ns = (uint32_t)plan.send_idx.size();
  PackArgs pa{};
  int tot = 0;
  for (const HField& f : fields) {
    if (pa.nf == 8) throw std::logic_error("halo: too many fields");
    pa.f[pa.nf++] = PackField{f.ptr, f.comps, (uint32_t)((size_t)ns * tot)};
    tot += f.comps;
  }
  if (tot > plan.max_comps) throw std::logic_error("halo: stage buffer too small");
  pa.idx = plan.d_send_idx;
  pa.n = ns;
  pa.stage = plan.d_stage;
  if (!plan.all_direct) launch_pack(pa, stream);
  std::vector<Msg> msgs;
  for (const HaloPeer& h : plan.peers) {
    for (int f = 0; f < pa.nf; ++f) {
      const PackField& F = pa.f[f];
      Msg mm;
      mm.peer = h.rank;
      mm.sbuf = plan.all_direct ? F.src + (ptrdiff_t)h.direct * F.comps
                                : plan.d_stage + F.stage_off + (size_t)h.send_off * F.comps;
      mm.sbytes = (size_t)h.send_cnt * F.comps * sizeof(float);
      mm.rbuf = const_cast<float*>(F.src) + (ptrdiff_t)h.recv_rel * F.comps;
      mm.rbytes = (size_t)h.recv_cnt * F.comps * sizeof(float);
      msgs.push_back(mm);
    }
  }
  CFD_HIP(hipEventRecord(hev_pack, stream));
  CFD_HIP(hipStreamWaitEvent(cstream, hev_pack, 0));
  halo_cat = comm_cat;
  comm->label = halo_cat;
  if (comm_prof) {
    hipEvent_t a = comm_event(), b = comm_event();
    CFD_HIP(hipEventRecord(a, cstream));
    comm->exchange(msgs, cstream);
    CFD_HIP(hipEventRecord(b, cstream));
    comm_recs.push_back({halo_cat, 1, a, b});
    CommTimes& t = comm_times[halo_cat];
    t.calls++;
    for (const Msg& mm : msgs) t.bytes += mm.sbytes;
  } else {
    comm->exchange(msgs, cstream);
  }
  CFD_HIP(hipEventRecord(hev_done, cstream));
}

// ghosts of the current FluidState slot: u, p (all = also d_p, grad_p)
void Solver::halo_state(bool all) {
  StateView& s = S();
  if (all)
    halo(cell_plan, {{(float*)s.u, 2}, {s.p, 1}, {s.dp, 1}, {(float*)s.gp, 2}});
  else
    halo(cell_plan, {{(float*)s.u, 2}, {s.p, 1}});
}

// Canonical reductions (kernels.hpp): one GPU hands the chunk partials to the
// finishing kernel; a distributed rank reduces its own segments, all-gathers
// the segment values, and every rank finishes the same global tree.
RedSrc Solver::combine(const float* part, int nvec) {
  RedSrc r;
  r.G = red.G / red.U;  // units per segment
  r.nseg = red.nseg;
  r.nvec = (uint32_t)nvec;
  if (!dist()) {
    r.p = part;
    r.stride = pstride;
    r.nchunks = nunits;
    return r;
  }
  launch_seg_reduce(part, pstride, nunits, r.G, nvec, red_local, maxseg, stream);
  const size_t bytes = (size_t)nvec * maxseg * sizeof(float);
  timed_gather(kCommReduceGather, bytes, [&] { comm->allgather(red_local, red_gather, bytes, stream); });
  r.p = red_gather;
  r.stride = maxseg;
  r.seg_src = d_seg_src;
  return r;
}

RedSrcD Solver::combine_d(const double* part, int nvec, double* local, double* gather) {
  if (!local) {
    local = red_local_d;
    gather = red_gather_d;
  }
  RedSrcD r;
  r.G = red.G / red.U;  // units per segment
  r.nseg = red.nseg;
  r.nvec = (uint32_t)nvec;
  if (!dist()) {
    r.p = part;
    r.stride = pstride;
    r.nchunks = nunits;
    return r;
  }
  launch_seg_reduce_d(part, pstride, nunits, r.G, nvec, local, maxseg, stream);
  const size_t bytes = (size_t)nvec * maxseg * sizeof(double);
  timed_gather(kCommReduceGather, bytes, [&] { comm->allgather(local, gather, bytes, stream); });
  r.p = gather;
  r.stride = maxseg;
  r.seg_src = d_seg_src;
  return r;
}

// ------------------------------------------------------------------ kernels
void Solver::rotate() {  // coupled_solver.rs:43-71
  step_index = (step_index + 1) % 3;
  static const int tab[3][3] = {{0, 1, 2}, {2, 0, 1}, {1, 2, 0}};
  i_state = tab[step_index][0];
  i_old = tab[step_index][1];
  i_old_old = tab[step_index][2];
}

void Solver::prepare() {
  PrepareArgs a;
  a.N = N;
  a.c = constants;
  a.fs = fs;
  a.vol = d_vol;
  a.st = S();
  a.dp_out = dp_scratch;
  a.gp_out = gp_scratch;
  a.flux_s = flux_s;
  a.grad_u = grad_u;
  a.grad_v = grad_v;
  if (ref_racy) {  // test mode: in place, workgroups in order, the owners' fluxes
    a.dp_out = S().dp;
    a.gp_out = S().gp;
    launch_prepare_ordered(a, d_flux_mirror, (uint32_t)((size_t)topo.wf * N), stream);
    check_launch("prepare (reference semantics)");
    return;
  }
  launch_prepare(a, stream);
  check_launch("prepare");
  // commit d_p / grad_p (snapshot semantics): swap the scratch into the slot
  std::swap(S().dp, dp_scratch);
  std::swap(S().gp, gp_scratch);
  if (dist())  // assemble reads the neighbours' new d_p (and gradients for SOU/QUICK)
    halo(cell_plan, {{S().dp, 1}, {(float*)S().gp, 2}, {(float*)grad_u, 2}, {(float*)grad_v, 2}});
}

void Solver::assemble() {
  AssembleArgs a;
  a.N = N;
  a.ld = topo.ld;
  a.c = constants;
  a.fs = fs;
  a.vol = d_vol;
  a.st = S();
  a.u_old = ring[i_old].u;
  a.u_old_old = ring[i_old_old].u;
  a.flux_s = flux_s;
  a.grad_u = grad_u;
  a.grad_v = grad_v;
  a.srank_diag = d_sdrank;
  a.cslot_diag = d_tdrank8;
  a.cval_a = cval_a;
  a.cval_g = cval_g;
  a.cdiag2 = cdiag2;
  a.sval = sval;
  a.rhs = rhs;
  a.dinv_uv = dinv_uv;
  a.dinv_p = dinv_p;
  launch_assemble(a, stream);
  check_launch("assemble");
  if (dist()) halo(cell_plan, {{dinv_uv, 1}});  // the Schur prediction reads neighbours' D_u^-1
}

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
  ev_iter.resize(2);  // the two pinned residual slots (Solver::solve)
  for (auto& e : ev_iter) CFD_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  fgmres_ready = true;
}

std::vector<uint64_t> Solver::allgather_u64(uint64_t mine) {
  std::vector<uint64_t> all(R, mine);
  if (!dist()) return all;
  if (!d_u64) d_u64 = arena.alloc<uint64_t>((size_t)R + 1);
  CFD_HIP(hipMemcpyAsync(d_u64, &mine, sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  comm->allgather(d_u64, d_u64 + 1, sizeof(uint64_t), stream);
  CFD_HIP(hipMemcpyAsync(all.data(), d_u64 + 1, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  sync();
  return all;
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

void Solver::set_reference_semantics(int flags) {
  if (flags & ~(1 | 2 | 4 | 8))
    throw std::invalid_argument("reference semantics on the GPU: flags 1 (in-place smoother), 2 (racy prepare), "
                                "4 (reduction order), 8 (restrict clamp) only");
  if (flags && dist()) throw std::invalid_argument("reference semantics: one GPU only");
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

float Solver::norm_blocking(const float* v, int mode, int slot) {
  norm_launch(v, mode, slot);
  sync();
  return h_pin[slot];
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
    CoupledMatrix A = cmat();
    A.r0 = a;
    A.r1 = b;
    A.r2 = a2;
    A.r3 = b2;
    launch_spmv(A, x, basis, stream, rhs, nt(8));  // V0 = 1 * b + -1 * (A x) as the SpMV stores it
  });
  norm_launch(basis, 2, 1);
}

// complete the lagged FGMRES residual read, if one is pending (async_buffer.rs)
void Solver::flush_inner() {
  if (inner.pending < 0) return;
  CFD_HIP(hipEventSynchronize(ev_iter[inner.pending]));
  inner.last = h_pin[64 + inner.pending];
  inner.has_last = true;
  inner.pending = -1;
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
    CoupledMatrix A = cmat();
    A.r0 = a;
    A.r1 = b;
    A.r2 = a2;
    A.r3 = b2;
    launch_spmv(A, zj, w, stream, nullptr, nt(8));
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
      // iteration, restart or solve: the reader is never reset)
      const int wslot = inner.pending == 0 ? 1 : 0;
      run_iteration(j, fixed ? nullptr : d_pin + 64 + wslot, fixed ? 0 : 1 + wslot);
      if (fixed) continue;
      // async residual read with the lag model (async_buffer.rs)
      flush_inner();
      // k_norm_givens wrote resid_hist[j] into h_pin[64 + wslot]; the event orders the read
      CFD_HIP(hipEventRecord(ev_iter[wslot], stream));
      bool have = false;
      float check = 0.0f;
      if (lag == 0) {
        CFD_HIP(hipEventSynchronize(ev_iter[wslot]));
        inner.last = h_pin[64 + wslot];
        inner.has_last = true;
        have = true;
        check = inner.last;
      } else {
        have = inner.has_last;
        check = inner.last;
        inner.pending = wslot;
      }
      if (have && (total % 10 == 0 || check < tol * rhs_norm))
        log("FGMRES iter %u: residual = %s (target %s)\n", total, e2(check).c_str(), e2(tol * rhs_norm).c_str());
      if (have && check < tol * rhs_norm) {
        converged = true;
        break;
      }
    }
    launch_solve_triangular(H, g, y, basis_size, m1, stream);
    launch_update_x(x, zvec, stride, y, basis_size, n, stream, small_forms);  // 0: the streaming form
    check_launch("FGMRES solution update");
    if (converged) {  // async_reader.flush()
      flush_inner();
      final_resid = inner.last;
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

// Reference reduction order (test mode): coupled_solver.rs:504-545 literally,
// on the host -- the AoS FluidState view (8 floats per cell: u, v, p, d_p,
// grad_p, grad_component = 0) read at floats 2i, 2i + 1 (the stride bug) and
// serial f64 loops.  tot: evolution, sum u, sum v, sum u^2, sum v^2.
void Solver::evolution_reference(double tot[5]) {
  auto aos = [&](const StateView& v, std::vector<float>& out) {
    std::vector<float2> u(N), gp(N);
    std::vector<float> p(N), dp(N);
    CFD_HIP(hipMemcpyAsync(u.data(), v.u, N * sizeof(float2), hipMemcpyDeviceToHost, stream));
    CFD_HIP(hipMemcpyAsync(p.data(), v.p, N * sizeof(float), hipMemcpyDeviceToHost, stream));
    CFD_HIP(hipMemcpyAsync(dp.data(), v.dp, N * sizeof(float), hipMemcpyDeviceToHost, stream));
    CFD_HIP(hipMemcpyAsync(gp.data(), v.gp, N * sizeof(float2), hipMemcpyDeviceToHost, stream));
    sync();
    out.assign(8 * (size_t)N, 0.0f);
    for (size_t c = 0; c < N; ++c) {
      float* r = out.data() + 8 * c;
      r[0] = u[c].x;
      r[1] = u[c].y;
      r[2] = p[c];
      r[3] = dp[c];
      r[4] = gp[c].x;
      r[5] = gp[c].y;
    }
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

// check_evolution (coupled_solver.rs:501-580), statistics on the GPU.  The
// stride bug (§0.1-12) makes index i read record i >> 2: a distributed rank
// first fetches the records [ev_a, ev_b) its indices read from their owners.
void Solver::check_evolution() {
  StateView var = S();
  uint64_t gbase = 0, rec0 = 0;
  if (dist()) {
    std::vector<Msg> msgs;
    StateView& cur = S();
    const uint64_t c0 = topo.c0, c1 = topo.c1;
    auto add = [&](int q, bool send, uint64_t lo, uint64_t hi) {
      const size_t n = hi - lo;
      if (send) {  // owned records [lo, hi) to rank q
        const size_t o = lo - c0;
        msgs.push_back({q, cur.u + o, n * sizeof(float2), nullptr, 0});
        msgs.push_back({q, cur.p + o, n * sizeof(float), nullptr, 0});
        msgs.push_back({q, cur.dp + o, n * sizeof(float), nullptr, 0});
        msgs.push_back({q, cur.gp + o, n * sizeof(float2), nullptr, 0});
      } else {  // records [lo, hi) of rank q
        const size_t o = lo - ev_a;
        msgs.push_back({q, nullptr, 0, evrec.u + o, n * sizeof(float2)});
        msgs.push_back({q, nullptr, 0, evrec.p + o, n * sizeof(float)});
        msgs.push_back({q, nullptr, 0, evrec.dp + o, n * sizeof(float)});
        msgs.push_back({q, nullptr, 0, evrec.gp + o, n * sizeof(float2)});
      }
    };
    for (int q = 0; q < R; ++q) {
      const uint64_t qa = starts[q] >> 2, qb = ((starts[q + 1] - 1) >> 2) + 1;  // q's record range
      // what q reads from me
      const uint64_t slo = std::max(qa, c0), shi = std::min(qb, c1);
      // what I read from q
      const uint64_t rlo = std::max(ev_a, starts[q]), rhi = std::min(ev_b, starts[q + 1]);
      if (q == rk) {
        if (rlo < rhi) {
          const size_t n = rhi - rlo, so = rlo - c0, ro = rlo - ev_a;
          CFD_HIP(hipMemcpyAsync(evrec.u + ro, cur.u + so, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
          CFD_HIP(hipMemcpyAsync(evrec.p + ro, cur.p + so, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
          CFD_HIP(hipMemcpyAsync(evrec.dp + ro, cur.dp + so, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
          CFD_HIP(hipMemcpyAsync(evrec.gp + ro, cur.gp + so, n * sizeof(float2), hipMemcpyDeviceToDevice, stream));
        }
        continue;
      }
      if (slo < shi) add(q, true, slo, shi);
      if (rlo < rhi) add(q, false, rlo, rhi);
    }
    comm->label = kCommStateHalo;
    comm->exchange(msgs, stream);
    var = evrec;
    gbase = topo.c0;
    rec0 = ev_a;
  }
  double tot[5];
  if (ref_red) {
    evolution_reference(tot);
  } else {
    launch_evolution_partial(S(), prev, have_prev ? 1 : 0, N, var, gbase, rec0, red.U, partial_d, pstride, stream);
    double* out5 = partial_d + 5 * (size_t)pstride;
    launch_evolution_final(combine_d(partial_d, 5), out5, stream);
    check_launch("check_evolution");
    CFD_HIP(hipMemcpyAsync(tot, out5, sizeof(tot), hipMemcpyDeviceToHost, stream));
  }
  copy_state(S(), prev, 0, N, stream);
  sync();
  const double nn = (double)NG;
  const double mean_u = tot[1] / nn, mean_v = tot[2] / nn;
  const double var_u = std::fmax(tot[3] / nn - mean_u * mean_u, 0.0);
  const double var_v = std::fmax(tot[4] / nn - mean_v * mean_v, 0.0);
  variance_history.push_back({var_u, var_v});
  if (variance_history.size() > 10) variance_history.erase(variance_history.begin());
  const double evo = have_prev ? std::sqrt(tot[0] / nn) : std::numeric_limits<double>::max();
  have_prev = true;
  if (evo < 1e-6) {
    if (var_u < 1e-10 && var_v < 1e-10) {
      info.degenerate_count++;
      info.steady_state_count = 0;
    } else {
      info.steady_state_count++;
      info.degenerate_count = 0;
    }
  } else {
    info.degenerate_count = 0;
    info.steady_state_count = 0;
  }
  if (info.degenerate_count > 10) {
    log("Solution is degenerate: Velocity field is uniform and not evolving. Variance U: %s, V: %s\n",
        e2(var_u).c_str(), e2(var_v).c_str());
    info.should_stop = 1;
  }
  if (info.steady_state_count > 10) {
    log("Steady state reached. Evolution diff: %s\n", e2(evo).c_str());
    info.should_stop = 1;
  }
}

void Solver::step() {  // coupled_solver.rs:33-499
  const Range range("cfd step");
  CFD_HIP(hipSetDevice(device));
  // opt-in deviation from the frozen hierarchy
  if (cfg.amg_rebuild_interval > 0 && amg_built && amg_age >= (uint32_t)cfg.amg_rebuild_interval) {
    // numeric re-setup over the kept structure when the device setup built it
    // (CFD_AMG_SETUP=rebuild: full rebuild; both give the same hierarchy)
    const char* se = knob(Knob::AmgSetup);  // "rebuild": a full setup instead of the refresh
    if (amg_setup_path == 2 && !amg_refresh.empty() && !(se && std::strcmp(se, "rebuild") == 0))
      amg_refresh_pending = true;
    else
      drop_amg();
  }
  rotate();
  constants.component = 0;
  last_step_dt = constants.dt;  // host only: cfd_scalar_advance(dt <= 0) advances by the step's dt
  const int fault_rank = debug_fault_after_prepare;  // test hook, one step only
  debug_fault_after_prepare = -1;
  if (dist()) halo_state(true);  // the rotated slot's ghosts (last written 3 steps ago)
  prepare();
  if (fault_rank == rk) throw std::runtime_error("injected fault after prepare");
  const bool fixed = cfg.fixed_outer > 0;
  const int max_iters = fixed ? cfg.fixed_outer : std::max(cfg.n_outer_correctors, 10);
  const double tol_u = 1e-5, tol_p = 1e-4;
  double prev_u = std::numeric_limits<double>::max(), prev_p = std::numeric_limits<double>::max();
  LagReader outer;  // reset per step (coupled_solver.rs:119-121)
  float last_u = 0.0f, last_p = 0.0f;
  int pend = -1;
  info.total_linear_iterations = 0;
  for (int iter = 0; iter < max_iters; ++iter) {
    const Range outer_range("picard iteration");
    log("Coupled Iteration: %d\n", iter + 1);
    if (iter > 0 || constants.scheme != 0) prepare();
    assemble();
    const cfd_linear_stats ls = solve();
    log("Coupled linear solve: %u iterations, residual %s, converged=%s\n", ls.iterations, e2(ls.residual).c_str(),
        tf(ls.converged));
    info.stats_p = ls;
    info.total_linear_iterations += ls.iterations;
    if (std::isnan(ls.residual)) throw std::domain_error("Coupled Linear Solver Diverged: NaN detected in linear residual");
    // the final max-diff pair also lands in this iteration's pinned host slot
    // (h_pin + 32 + 2 (iter & 1)): the lagged read below needs no copy launch
    uint32_t* host_slot = reinterpret_cast<uint32_t*>(d_pin + 32 + 2 * (iter & 1));
    launch_update_fields(N, constants.alpha_u, constants.alpha_p, x, S().u, S().p, blockmax, maxbits,
                         dist() ? nullptr : host_slot, stream);
    check_launch("update_fields");
    if (dist()) {
      halo_state(false);  // the next prepare reads neighbours' u, p
      timed_gather(kCommReduceGather, 2 * sizeof(uint32_t),
                   [&] { comm->allgather(maxbits, mx_gather, 2 * sizeof(uint32_t), stream); });
      launch_max_combine(mx_gather, R, maxbits, host_slot, stream);
    }
    if (iter == 0) {
      info.outer_residual_u = std::numeric_limits<float>::max();
      info.outer_residual_p = std::numeric_limits<float>::max();
      info.outer_iterations = 1;
      continue;
    }
    // async max-diff read (coupled_solver.rs:396-479) under the lag model
    float* slot = h_pin + 32 + 2 * (iter & 1);
    if (pend >= 0) {
      CFD_HIP(hipEventSynchronize(ev_outer[pend]));
      std::memcpy(&last_u, h_pin + 32 + 2 * pend, 4);
      std::memcpy(&last_p, h_pin + 32 + 2 * pend + 1, 4);
      outer.has_last = true;
      pend = -1;
    }
    CFD_HIP(hipEventRecord(ev_outer[iter & 1], stream));  // orders the read of slot
    bool have = false;
    float cu = 0.0f, cp = 0.0f;
    if (cfg.convergence_lag == 0) {
      CFD_HIP(hipEventSynchronize(ev_outer[iter & 1]));
      std::memcpy(&cu, slot, 4);
      std::memcpy(&cp, slot + 1, 4);
      have = true;
    } else {
      have = outer.has_last;
      cu = last_u;
      cp = last_p;
      pend = iter & 1;
    }
    if (!have) continue;
    const double du = cu, dp = cp;
    if (std::isnan(du) || std::isnan(dp)) throw std::domain_error("Coupled Solver Diverged: NaN detected in outer residuals");
    info.outer_residual_u = cu;
    info.outer_residual_p = cp;
    info.outer_iterations = iter + 1;
    log("Coupled Residuals - U: %s, P: %s\n", e2(du).c_str(), e2(dp).c_str());
    if (!fixed) {
      if (du < tol_u && dp < tol_p) {
        log("Coupled Solver Converged in %d iterations\n", iter + 1);
        break;
      }
      const double rel_u = (std::isfinite(prev_u) && std::fabs(prev_u) > 1e-14) ? std::fabs((du - prev_u) / prev_u)
                                                                                : std::numeric_limits<double>::infinity();
      const double rel_p = (std::isfinite(prev_p) && std::fabs(prev_p) > 1e-14) ? std::fabs((dp - prev_p) / prev_p)
                                                                                : std::numeric_limits<double>::infinity();
      if (rel_u < 1e-2 && rel_p < 1e-2 && iter > 2) {
        log("Coupled solver stagnated at iter %d: U=%s, P=%s\n", iter + 1, e2(du).c_str(), e2(dp).c_str());
        break;
      }
    }
    prev_u = du;
    prev_p = dp;
  }
  constants.time += constants.dt;
  if (amg_built) ++amg_age;
  check_evolution();
}

// ------------------------------------------------------------------ debug
void Solver::debug_prepare_assemble(bool asmb) {
  CFD_HIP(hipSetDevice(device));
  constants.component = 0;
  prepare();
  if (asmb) assemble();
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

// ------------------------------------------------------------- accounting
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
  const double prep = 40 * S + 60 * Nn;                    // 9 slot arrays + flux out; cell state in, gradients out
  const double asmb = 32 * S + 20 * Sint + 78 * Nn;        // 8 slot arrays; 3x3 block + Poisson entry out
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
  const double prep = 84 * Nn + 4 * Sfaces + 36 * Fn;
  const double asmb = 68 * Nn + 8 * Sfaces + 36 * Fn + 40 * nnz_s;
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
