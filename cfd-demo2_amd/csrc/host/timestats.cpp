// Time statistics and the monitor history (include/cfd2_amd.h "Time-averaged
// fields" and "Monitor history"; kernels.hpp "timestats.hip"): the f64 planes
// with their totals, and the ring of probe samples and flow diagnostics.
// Read-only on the solver's state by their type: the solver arrives as a const
// FlowView, pointers to const, and this file does not see the Solver.  Every
// buffer lives in the modules' own arenas.
#include <cmath>
#include <cstring>

#include "modules.hpp"

namespace cfd2 {

void TimeStats::need(const char* what) const {
  if (!planes) throw std::invalid_argument(std::string(what) + ": time statistics are not enabled (cfd_tstats_enable)");
}

void TimeStats::disable(const FlowView& flow) {
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();
  arena.release();
  planes = nullptr;
  np = 0;
  ld = 0;
  m2 = scalars = false;
  nf = 0;
  W = 0.0;
  samples = 0;
}

void TimeStats::enable(const FlowView& flow, const cfd_tstats_config* cfg) {
  const int32_t sm = cfg ? cfg->second_moments : 1, sc = cfg ? cfg->scalars : 1;
  if ((sm != 0 && sm != 1) || (sc != 0 && sc != 1))
    throw std::invalid_argument("time statistics: second_moments and scalars must be 0 or 1");
  disable(flow);
  const uint32_t fields = sc ? (uint32_t)flow.nf : 0u;
  const uint32_t count = tstats_planes(sm != 0, fields);
  const size_t stride = ((size_t)flow.N + 31) / 32 * 32;
  double* buf = arena.alloc<double>((size_t)count * stride);
  CFD_HIP(hipMemsetAsync(buf, 0, (size_t)count * stride * sizeof(double), flow.stream));
  flow.sync();
  planes = buf;
  np = count;
  ld = stride;
  m2 = sm != 0;
  scalars = sc != 0;
  nf = fields;
}

void TimeStats::reset(const FlowView& flow) {
  need("cfd_tstats_reset");
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemsetAsync(planes, 0, (size_t)np * ld * sizeof(double), flow.stream));
  W = 0.0;
  samples = 0;
}

void TimeStats::accumulate(const FlowView& flow, float weight) {
  need("cfd_tstats_accumulate");
  if (!std::isfinite(weight)) throw std::invalid_argument("cfd_tstats_accumulate: the weight must be finite");
  if (scalars && (uint32_t)flow.nf != nf)
    throw std::invalid_argument("cfd_tstats_accumulate: " + std::to_string(flow.nf) + " scalar fields are enabled, the "
                                "statistics were enabled with " + std::to_string(nf) + " (cfd_tstats_enable again)");
  if (!(weight > 0.0f)) {
    if (!(flow.last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_tstats_accumulate: weight <= 0 asks for the dt of the last cfd_step, and there was none");
    weight = flow.last_step_dt;
  }
  const Range range("time statistics");
  CFD_HIP(hipSetDevice(flow.device));
  const double w = (double)weight, Wn = W + w;
  TimeStatsArgs a{};
  a.N = flow.N;
  a.nf = nf;
  a.u = flow.u;
  a.p = flow.p;
  a.planes = planes;
  a.ld = ld;
  a.w = w;
  a.r = w / Wn;
  for (uint32_t f = 0; f < nf; ++f) a.phi[f] = flow.field[f].phi;
  launch_tstats(a, m2, flow.stream);
  flow.check_launch("time statistics");
  W = Wn;
  samples += 1;
}

int TimeStats::plane_of(int kind, int scalar_index, bool* covariance) const {
  if (kind < 0 || kind > 10) throw std::invalid_argument("time statistics: kind must be 0..10");
  const bool cov = (kind >= 3 && kind <= 6) || kind >= 8;
  if (covariance) *covariance = cov;
  if (kind <= 2) return kind;
  if (kind <= 6) {
    if (!m2) throw std::invalid_argument("time statistics: kind " + std::to_string(kind) + " needs second_moments");
    return kind;
  }
  if (scalar_index < 0 || (uint32_t)scalar_index >= nf)
    throw std::invalid_argument("time statistics: scalar index " + std::to_string(scalar_index) + " outside [0, " +
                                std::to_string(nf) + ") of the fields the statistics hold");
  if (kind >= 9 && !m2)
    throw std::invalid_argument("time statistics: kind " + std::to_string(kind) + " needs second_moments");
  const int base = 3 + (m2 ? 4 : 0) + scalar_index * (m2 ? 4 : 2);
  return base + (kind - 7);  // mean, M_ff, M_uf, M_vf
}

void TimeStats::get(const FlowView& flow, int kind, int scalar_index, double* out) {
  need("cfd_tstats_get");
  bool cov = false;
  const int q = plane_of(kind, scalar_index, &cov);
  if (!(W > 0.0)) throw std::invalid_argument("cfd_tstats_get: no sample yet (the total weight is 0)");
  raw(flow, (uint32_t)q, out, nullptr);
  if (cov)
    for (uint32_t i = 0; i < flow.N; ++i) out[i] = out[i] / W;
}

void TimeStats::raw(const FlowView& flow, uint32_t plane, double* out, const double* in) {
  need("cfd_tstats_raw");
  if (plane >= np)
    throw std::invalid_argument("time statistics: plane " + std::to_string(plane) + " outside [0, " + std::to_string(np) + ")");
  CFD_HIP(hipSetDevice(flow.device));
  double* d = planes + (size_t)plane * ld;
  if (out)
    CFD_HIP(hipMemcpyAsync(out, d, (size_t)flow.N * sizeof(double), hipMemcpyDeviceToHost, flow.stream));
  else
    CFD_HIP(hipMemcpyAsync(d, in, (size_t)flow.N * sizeof(double), hipMemcpyHostToDevice, flow.stream));
  flow.sync();
}

void TimeStats::set_totals(const FlowView&, uint64_t samples_in, double W_in) {
  need("cfd_tstats_raw_set_totals");
  if (!std::isfinite(W_in) || W_in < 0.0) throw std::invalid_argument("cfd_tstats_raw_set_totals: the total weight must be finite and >= 0");
  samples = samples_in;
  W = W_in;
}

void TimeStats::info(const FlowView&, uint64_t* samples_out, double* total_weight, uint32_t* planes_out) const {
  need("cfd_tstats_info");
  if (samples_out) *samples_out = samples;
  if (total_weight) *total_weight = W;
  if (planes_out) *planes_out = np;
}

// ------------------------------------------------------------------ monitor
void Monitor::need(const char* what) const {
  if (cap == 0) throw std::invalid_argument(std::string(what) + ": the monitor is not enabled (cfd_monitor_enable)");
}

void Monitor::disable(const FlowView& flow) {
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();
  arena.release();
  cap = P = ns = 0;
  diag = false;
  total = 0;
  cells = nullptr;
  time = probe = nullptr;
  dres = nullptr;
  faces.clear();
}

void Monitor::enable(const FlowView& flow, uint32_t capacity, uint32_t num_probes, const uint32_t* probe_cells,
                     bool with_diag) {
  if (capacity < 1 || capacity > (1u << 20)) throw std::invalid_argument("monitor: capacity must be 1..2^20 samples");
  if (num_probes > 1024) throw std::invalid_argument("monitor: num_probes must be 0..1024");
  if (num_probes && !probe_cells) throw std::invalid_argument("monitor: null probe cells");
  for (uint32_t k = 0; k < num_probes; ++k)
    if (probe_cells[k] >= flow.N)
      throw std::invalid_argument("monitor: probe " + std::to_string(k) + " is cell " + std::to_string(probe_cells[k]) +
                                  ", outside [0, " + std::to_string(flow.N) + ")");
  disable(flow);
  const uint32_t fields = (uint32_t)flow.nf;
  cells = arena.upload(std::vector<uint32_t>(probe_cells, probe_cells + num_probes), flow.stream);
  time = arena.alloc<float>(2 * (size_t)capacity);
  probe = arena.alloc<float>((size_t)capacity * num_probes * (3 + fields));
  if (with_diag) {
    dres = arena.alloc<uint64_t>((size_t)capacity * kMonitorDiagWords);
    faces.assign(capacity, 0u);
  }
  flow.sync();  // the upload read a host vector that ends here
  cap = capacity;
  P = num_probes;
  ns = fields;
  diag = with_diag;
}

void Monitor::record_check(const FlowView& flow) const {
  need("cfd_monitor_record");
  if ((uint32_t)flow.nf != ns)
    throw std::invalid_argument("cfd_monitor_record: " + std::to_string(flow.nf) + " scalar fields are enabled, the "
                                "monitor was enabled with " + std::to_string(ns) + " (cfd_monitor_enable again)");
}

void Monitor::record(const FlowView& flow, const uint64_t* diag_res, const ForceRegion& region) {
  record_check(flow);
  CFD_HIP(hipSetDevice(flow.device));
  const size_t slot = (size_t)(total % cap);
  if (diag) faces[slot] = region.faces;
  MonitorRecordArgs a{};
  a.P = P;
  a.ns = ns;
  a.cells = cells;
  a.u = flow.u;
  a.p = flow.p;
  for (uint32_t f = 0; f < ns; ++f) a.phi[f] = flow.field[f].phi;
  a.time = flow.constants.time;
  a.dt = flow.last_step_dt;
  a.time_out = time + 2 * slot;
  a.probe_out = probe + slot * P * (3 + ns);
  a.diag_res = diag_res;
  a.diag_out = diag ? dres + slot * kMonitorDiagWords : nullptr;
  launch_monitor_record(a, flow.stream);
  flow.check_launch("monitor record");
  total += 1;
}

void Monitor::get(const FlowView& flow, uint64_t first, uint64_t count, float* time_out, float* dt, float* probes,
                  cfd_flow_diag* diag_out) {
  need("cfd_monitor_get");
  const uint64_t held = std::min<uint64_t>(total, cap);
  if (first > held || count > held - first)
    throw std::invalid_argument("cfd_monitor_get: first + count exceeds the " + std::to_string(held) + " samples held");
  if (count == 0) return;
  CFD_HIP(hipSetDevice(flow.device));
  const size_t pw = (size_t)P * (3 + ns);
  std::vector<float> ht(2 * (size_t)count);
  std::vector<uint64_t> hd(diag && diag_out ? (size_t)count * kMonitorDiagWords : 0);
  // held sample j is sample number total - held + j, in slot (that number) % capacity: at most two runs of slots
  const uint64_t k0 = total - held + first;
  for (uint64_t done = 0; done < count;) {
    const size_t slot = (size_t)((k0 + done) % cap);
    const size_t run = (size_t)std::min<uint64_t>(count - done, cap - slot);
    CFD_HIP(hipMemcpyAsync(ht.data() + 2 * done, time + 2 * slot, run * 2 * sizeof(float), hipMemcpyDeviceToHost, flow.stream));
    if (probes && pw)
      CFD_HIP(hipMemcpyAsync(probes + done * pw, probe + slot * pw, run * pw * sizeof(float), hipMemcpyDeviceToHost, flow.stream));
    if (!hd.empty())
      CFD_HIP(hipMemcpyAsync(hd.data() + done * kMonitorDiagWords, dres + slot * kMonitorDiagWords,
                             run * kMonitorDiagWords * sizeof(uint64_t), hipMemcpyDeviceToHost, flow.stream));
    done += run;
  }
  flow.sync();
  for (uint64_t j = 0; j < count; ++j) {
    if (time_out) time_out[j] = ht[2 * j];
    if (dt) dt[j] = ht[2 * j + 1];
    if (!diag_out) continue;
    if (!diag) {
      std::memset(&diag_out[j], 0, sizeof(cfd_flow_diag));
      continue;
    }
    const uint64_t* h = hd.data() + j * kMonitorDiagWords;
    flow_diag_decode(h, h + 6, faces[(size_t)((k0 + j) % cap)], &diag_out[j]);
  }
}

void Monitor::count(const FlowView&, uint64_t* total_out, uint64_t* held) const {
  need("cfd_monitor_count");
  if (total_out) *total_out = total;
  if (held) *held = std::min<uint64_t>(total, cap);
}

void Monitor::info(const FlowView&, uint32_t* capacity, uint32_t* num_probes, uint32_t* scalar_fields,
                   int32_t* with_diag) const {
  need("cfd_monitor_info");
  if (capacity) *capacity = cap;
  if (num_probes) *num_probes = P;
  if (scalar_fields) *scalar_fields = ns;
  if (with_diag) *with_diag = diag ? 1 : 0;
}

}  // namespace cfd2
