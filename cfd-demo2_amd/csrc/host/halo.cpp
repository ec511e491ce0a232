// Distributed plumbing of the HIP solver: halo exchanges of per-cell fields
// over a HaloPlan (comm stream, overlapped by Solver::overlapped), their timing,
// and the all-gathers that finish the canonical reductions on every rank.
#include <type_traits>

#include "solver_impl.hpp"

namespace cfd2 {

void Solver::make_plan_buffers(HaloPlan& p, int max_comps) {
  p.d_send_idx = arena.upload(p.send_idx, stream);
  p.max_comps = max_comps;
  p.d_stage = arena.alloc<float>(p.send_idx.size() * (size_t)max_comps + 1);
}

// Halo exchange of per-cell fields over `plan`: pack the rows the peers need,
// then one grouped transfer per (peer, field) straight into the ghost slots.
void Solver::halo(HaloPlan& plan, std::initializer_list<HField> fields) {
  if (!dist()) return;
  halo_begin(plan, fields);
  halo_end();
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

// ghosts of the current FluidState slot: u, p (all = also d_p, grad_p)
void Solver::halo_state(bool all) {
  HField f[4];
  int nf = 0;
  for_each_field(S(), [&](float* base, int comps) { f[nf++] = {base, comps}; });
  if (all)
    halo(cell_plan, {f[0], f[1], f[2], f[3]});
  else
    halo(cell_plan, {f[0], f[1]});
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

// Canonical reductions (kernels.hpp): one GPU hands the chunk partials to the
// finishing kernel; a distributed rank reduces its own segments, all-gathers
// the segment values, and every rank finishes the same global tree.
template <class T>
RedSrcT<T> Solver::combine(const T* part, int nvec, T* local, T* gather) {
  if (!dist()) return sums().src(part, nvec);
  RedSrcT<T> r;
  r.G = red.G / red.U;  // units per segment
  r.nseg = red.nseg;
  r.nvec = (uint32_t)nvec;
  if constexpr (std::is_same<T, double>::value) {
    if (!local) {
      local = red_local_d;
      gather = red_gather_d;
    }
    launch_seg_reduce_d(part, pstride, nunits, r.G, nvec, local, maxseg, stream);
  } else {
    if (!local) {
      local = red_local;
      gather = red_gather;
    }
    launch_seg_reduce(part, pstride, nunits, r.G, nvec, local, maxseg, stream);
  }
  const size_t bytes = (size_t)nvec * maxseg * sizeof(T);
  timed_gather(kCommReduceGather, bytes, [&] { comm->allgather(local, gather, bytes, stream); });
  r.p = gather;
  r.stride = maxseg;
  r.seg_src = d_seg_src;
  return r;
}
template RedSrcT<float> Solver::combine(const float*, int, float*, float*);
template RedSrcT<double> Solver::combine(const double*, int, double*, double*);

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

}  // namespace cfd2
