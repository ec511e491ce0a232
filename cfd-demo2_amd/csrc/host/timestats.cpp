// Time statistics and the monitor history (include/cfd2_amd.h "Time-averaged
// fields" and "Monitor history"; kernels.hpp "timestats.hip"): the f64 planes
// with their totals, and the ring of probe samples and flow diagnostics.
// Read-only on the solver's state; every buffer lives in the modules' own arenas.
#include <cmath>
#include <cstring>

#include "solver_impl.hpp"

namespace cfd2 {

namespace {
const char* kStatsOneGpu = "time statistics run on one GPU only: a distributed handle holds a part of the fields";
const char* kMonitorOneGpu = "the monitor runs on one GPU only: a distributed handle holds a part of the fields";
}  // namespace

void Solver::tstats_need(const char* what) const {
  if (dist()) throw std::invalid_argument(kStatsOneGpu);
  if (!ts_planes) throw std::invalid_argument(std::string(what) + ": time statistics are not enabled (cfd_tstats_enable)");
}

void Solver::tstats_disable() {
  if (dist()) throw std::invalid_argument(kStatsOneGpu);
  CFD_HIP(hipSetDevice(device));
  sync();
  ts_arena.release();
  ts_planes = nullptr;
  ts_np = 0;
  ts_ld = 0;
  ts_m2 = ts_scalars = false;
  ts_nf = 0;
  ts_W = 0.0;
  ts_samples = 0;
}

void Solver::tstats_enable(const cfd_tstats_config* cfg) {
  if (dist()) throw std::invalid_argument(kStatsOneGpu);
  const int32_t m2 = cfg ? cfg->second_moments : 1, sc = cfg ? cfg->scalars : 1;
  if ((m2 != 0 && m2 != 1) || (sc != 0 && sc != 1))
    throw std::invalid_argument("time statistics: second_moments and scalars must be 0 or 1");
  tstats_disable();
  const uint32_t nf = sc ? (uint32_t)sc_count : 0u;
  const uint32_t np = tstats_planes(m2 != 0, nf);
  const size_t ld = ((size_t)N + 31) / 32 * 32;
  double* planes = ts_arena.alloc<double>((size_t)np * ld);
  CFD_HIP(hipMemsetAsync(planes, 0, (size_t)np * ld * sizeof(double), stream));
  sync();
  ts_planes = planes;
  ts_np = np;
  ts_ld = ld;
  ts_m2 = m2 != 0;
  ts_scalars = sc != 0;
  ts_nf = nf;
}

void Solver::tstats_reset() {
  tstats_need("cfd_tstats_reset");
  CFD_HIP(hipSetDevice(device));
  CFD_HIP(hipMemsetAsync(ts_planes, 0, (size_t)ts_np * ts_ld * sizeof(double), stream));
  ts_W = 0.0;
  ts_samples = 0;
}

void Solver::tstats_accumulate(float weight) {
  tstats_need("cfd_tstats_accumulate");
  if (!std::isfinite(weight)) throw std::invalid_argument("cfd_tstats_accumulate: the weight must be finite");
  if (ts_scalars && (uint32_t)sc_count != ts_nf)
    throw std::invalid_argument("cfd_tstats_accumulate: " + std::to_string(sc_count) + " scalar fields are enabled, the "
                                "statistics were enabled with " + std::to_string(ts_nf) + " (cfd_tstats_enable again)");
  if (!(weight > 0.0f)) {
    if (!(last_step_dt > 0.0f))
      throw std::invalid_argument("cfd_tstats_accumulate: weight <= 0 asks for the dt of the last cfd_step, and there was none");
    weight = last_step_dt;
  }
  const Range range("time statistics");
  CFD_HIP(hipSetDevice(device));
  const double w = (double)weight, Wn = ts_W + w;
  TimeStatsArgs a{};
  a.N = N;
  a.nf = ts_nf;
  a.u = S().u;
  a.p = S().p;
  a.planes = ts_planes;
  a.ld = ts_ld;
  a.w = w;
  a.r = w / Wn;
  for (uint32_t f = 0; f < ts_nf; ++f) a.phi[f] = sc_field[f].phi;
  launch_tstats(a, ts_m2, stream);
  check_launch("time statistics");
  ts_W = Wn;
  ts_samples += 1;
}

int Solver::tstats_plane_of(int kind, int scalar_index, bool* covariance) const {
  if (kind < 0 || kind > 10) throw std::invalid_argument("time statistics: kind must be 0..10");
  const bool cov = (kind >= 3 && kind <= 6) || kind >= 8;
  if (covariance) *covariance = cov;
  if (kind <= 2) return kind;
  if (kind <= 6) {
    if (!ts_m2) throw std::invalid_argument("time statistics: kind " + std::to_string(kind) + " needs second_moments");
    return kind;
  }
  if (scalar_index < 0 || (uint32_t)scalar_index >= ts_nf)
    throw std::invalid_argument("time statistics: scalar index " + std::to_string(scalar_index) + " outside [0, " +
                                std::to_string(ts_nf) + ") of the fields the statistics hold");
  if (kind >= 9 && !ts_m2)
    throw std::invalid_argument("time statistics: kind " + std::to_string(kind) + " needs second_moments");
  const int base = 3 + (ts_m2 ? 4 : 0) + scalar_index * (ts_m2 ? 4 : 2);
  return base + (kind - 7);  // mean, M_ff, M_uf, M_vf
}

void Solver::tstats_get(int kind, int scalar_index, double* out) {
  tstats_need("cfd_tstats_get");
  bool cov = false;
  const int q = tstats_plane_of(kind, scalar_index, &cov);
  if (!(ts_W > 0.0)) throw std::invalid_argument("cfd_tstats_get: no sample yet (the total weight is 0)");
  tstats_raw((uint32_t)q, out, nullptr);
  if (cov)
    for (uint32_t i = 0; i < N; ++i) out[i] = out[i] / ts_W;
}

void Solver::tstats_raw(uint32_t plane, double* out, const double* in) {
  tstats_need("cfd_tstats_raw");
  if (plane >= ts_np)
    throw std::invalid_argument("time statistics: plane " + std::to_string(plane) + " outside [0, " + std::to_string(ts_np) + ")");
  CFD_HIP(hipSetDevice(device));
  double* d = ts_planes + (size_t)plane * ts_ld;
  if (out)
    CFD_HIP(hipMemcpyAsync(out, d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, stream));
  else
    CFD_HIP(hipMemcpyAsync(d, in, (size_t)N * sizeof(double), hipMemcpyHostToDevice, stream));
  sync();
}

void Solver::tstats_set_totals(uint64_t samples, double W) {
  tstats_need("cfd_tstats_raw_set_totals");
  if (!std::isfinite(W) || W < 0.0) throw std::invalid_argument("cfd_tstats_raw_set_totals: the total weight must be finite and >= 0");
  ts_samples = samples;
  ts_W = W;
}

// ------------------------------------------------------------------ monitor
void Solver::monitor_need(const char* what) const {
  if (dist()) throw std::invalid_argument(kMonitorOneGpu);
  if (mon_cap == 0) throw std::invalid_argument(std::string(what) + ": the monitor is not enabled (cfd_monitor_enable)");
}

void Solver::monitor_disable() {
  if (dist()) throw std::invalid_argument(kMonitorOneGpu);
  CFD_HIP(hipSetDevice(device));
  sync();
  mon_arena.release();
  mon_cap = mon_P = mon_ns = 0;
  mon_diag = false;
  mon_total = 0;
  mon_cells = nullptr;
  mon_time = mon_probe = nullptr;
  mon_dres = nullptr;
  mon_faces.clear();
}

void Solver::monitor_enable(uint32_t capacity, uint32_t num_probes, const uint32_t* cells, bool with_diag) {
  if (dist()) throw std::invalid_argument(kMonitorOneGpu);
  if (capacity < 1 || capacity > (1u << 20)) throw std::invalid_argument("monitor: capacity must be 1..2^20 samples");
  if (num_probes > 1024) throw std::invalid_argument("monitor: num_probes must be 0..1024");
  if (num_probes && !cells) throw std::invalid_argument("monitor: null probe cells");
  for (uint32_t k = 0; k < num_probes; ++k)
    if (cells[k] >= N)
      throw std::invalid_argument("monitor: probe " + std::to_string(k) + " is cell " + std::to_string(cells[k]) +
                                  ", outside [0, " + std::to_string(N) + ")");
  monitor_disable();
  const uint32_t ns = (uint32_t)sc_count;
  mon_cells = mon_arena.upload(std::vector<uint32_t>(cells, cells + num_probes), stream);
  mon_time = mon_arena.alloc<float>(2 * (size_t)capacity);
  mon_probe = mon_arena.alloc<float>((size_t)capacity * num_probes * (3 + ns));
  if (with_diag) {
    mon_dres = mon_arena.alloc<uint64_t>((size_t)capacity * kMonitorDiagWords);
    flow_diag_alloc(false);  // the record itself allocates nothing
    mon_faces.assign(capacity, 0u);
  }
  sync();  // the upload read a host vector that ends here
  mon_cap = capacity;
  mon_P = num_probes;
  mon_ns = ns;
  mon_diag = with_diag;
}

void Solver::monitor_record() {
  monitor_need("cfd_monitor_record");
  if ((uint32_t)sc_count != mon_ns)
    throw std::invalid_argument("cfd_monitor_record: " + std::to_string(sc_count) + " scalar fields are enabled, the "
                                "monitor was enabled with " + std::to_string(mon_ns) + " (cfd_monitor_enable again)");
  const Range range("monitor record");
  CFD_HIP(hipSetDevice(device));
  const size_t slot = (size_t)(mon_total % mon_cap);
  if (mon_diag) {
    flow_diag_device(false, true);
    mon_faces[slot] = region_faces;
  }
  MonitorRecordArgs a{};
  a.P = mon_P;
  a.ns = mon_ns;
  a.cells = mon_cells;
  a.u = S().u;
  a.p = S().p;
  for (uint32_t f = 0; f < mon_ns; ++f) a.phi[f] = sc_field[f].phi;
  a.time = constants.time;
  a.dt = last_step_dt;
  a.time_out = mon_time + 2 * slot;
  a.probe_out = mon_probe + slot * mon_P * (3 + mon_ns);
  a.diag_res = diag_res;
  a.diag_out = mon_diag ? mon_dres + slot * kMonitorDiagWords : nullptr;
  launch_monitor_record(a, stream);
  check_launch("monitor record");
  mon_total += 1;
}

void Solver::monitor_get(uint64_t first, uint64_t count, float* time, float* dt, float* probes, cfd_flow_diag* diag) {
  monitor_need("cfd_monitor_get");
  const uint64_t held = std::min<uint64_t>(mon_total, mon_cap);
  if (first > held || count > held - first)
    throw std::invalid_argument("cfd_monitor_get: first + count exceeds the " + std::to_string(held) + " samples held");
  if (count == 0) return;
  CFD_HIP(hipSetDevice(device));
  const size_t pw = (size_t)mon_P * (3 + mon_ns);
  std::vector<float> ht(2 * (size_t)count);
  std::vector<uint64_t> hd(mon_diag && diag ? (size_t)count * kMonitorDiagWords : 0);
  // held sample j is sample number mon_total - held + j, in slot (that number) % capacity: at most two runs of slots
  const uint64_t k0 = mon_total - held + first;
  for (uint64_t done = 0; done < count;) {
    const size_t slot = (size_t)((k0 + done) % mon_cap);
    const size_t run = (size_t)std::min<uint64_t>(count - done, mon_cap - slot);
    CFD_HIP(hipMemcpyAsync(ht.data() + 2 * done, mon_time + 2 * slot, run * 2 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (probes && pw)
      CFD_HIP(hipMemcpyAsync(probes + done * pw, mon_probe + slot * pw, run * pw * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (!hd.empty())
      CFD_HIP(hipMemcpyAsync(hd.data() + done * kMonitorDiagWords, mon_dres + slot * kMonitorDiagWords,
                             run * kMonitorDiagWords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    done += run;
  }
  sync();
  for (uint64_t j = 0; j < count; ++j) {
    if (time) time[j] = ht[2 * j];
    if (dt) dt[j] = ht[2 * j + 1];
    if (!diag) continue;
    if (!mon_diag) {
      std::memset(&diag[j], 0, sizeof(cfd_flow_diag));
      continue;
    }
    const uint64_t* h = hd.data() + j * kMonitorDiagWords;
    flow_diag_decode(h, h + 6, mon_faces[(size_t)((k0 + j) % mon_cap)], &diag[j]);
  }
}

}  // namespace cfd2
