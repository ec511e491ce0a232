// Volume penalisation (include/cfd2_amd.h "Arithmetic of volume penalisation"):
// the per-cell fields the PEN forms of prepare and assemble read, and the
// read-only force diagnostic.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "penalty.hpp"

namespace cfd2 {

PenaltyGeometry penalty_geometry(const Topology& t) {
  PenaltyGeometry g;
  const uint32_t N = t.N;
  for (uint32_t i = 0; i < N; ++i) {
    double gi = 0.0;
    for (uint32_t k = 0; k < t.nface[i]; ++k) {
      const size_t e = (size_t)k * N + i;
      const bool interior = t.fs_other[e] != kNoCell, outlet = (t.fs_meta[e] & kMetaBtypeMask) == 2u;
      if (interior || outlet) gi += (double)t.fs_area[e] / (double)t.fs_dist_a[e];
    }
    const double v = t.vol[i];
    if (i == 0) {
      g.vol_min = g.vol_max = v;
      g.g_min = gi;
    }
    g.vol_min = std::min(g.vol_min, v);
    g.vol_max = std::max(g.vol_max, v);
    g.g_min = std::min(g.g_min, gi);
  }
  return g;
}

double penalty_limit(const PenaltyGeometry& g, float density) {
  return (double)density * g.g_min * g.vol_min / (4.0 * 1e-14);
}

void Penalty::need(const char* what, bool dist, bool ref_mode) {
  if (dist) throw std::invalid_argument(std::string("volume penalisation runs on one GPU only: no ") + what + " on a distributed handle");
  if (ref_mode)
    throw std::invalid_argument(std::string("volume penalisation: no ") + what +
                                " in reference-semantics mode (the racy prepare and the in-place smoother have no such form)");
}

void Penalty::set(const FlowView& flow, const std::vector<float>& vol, double limit, const float* sigma,
                  const float* forch, const float* target, uint32_t count) {
  const uint32_t N = flow.N;
  if (count != 0 && count != N)
    throw std::invalid_argument("penalty: " + std::to_string(count) + " values for " + std::to_string(N) +
                                " cells (0 clears the field)");
  auto bad = [](const char* what, uint32_t i, const char* why) {
    throw std::invalid_argument(std::string("penalty: ") + what + " of cell " + std::to_string(i) + " " + why);
  };
  float smax = 0.0f, vmax = 0.0f;
  for (uint32_t i = 0; i < count; ++i) {
    if (!std::isfinite(sigma[i]) || sigma[i] < 0.0f) bad("sigma", i, "is not finite and >= 0");
    if (forch && (!std::isfinite(forch[i]) || forch[i] < 0.0f)) bad("forch", i, "is not finite and >= 0");
    if (target && (!std::isfinite(target[2 * (size_t)i]) || !std::isfinite(target[2 * (size_t)i + 1])))
      bad("the target", i, "is not finite");
    if ((double)vol[i] * (double)sigma[i] > limit)
      throw std::invalid_argument("penalty: vol * sigma of cell " + std::to_string(i) + " is " +
                                  std::to_string((double)vol[i] * (double)sigma[i]) + ", above this handle's limit " +
                                  std::to_string(limit) + " (the pressure row's diagonal would fall under 1e-14)");
    smax = std::max(smax, sigma[i]);
    vmax = std::max(vmax, vol[i]);
  }
  // the limit above is far below FLT_MAX / max(vol) on any mesh with a sane ratio of cell volumes, so this
  // fires only on a mesh whose largest cell is some 1e20 times its smallest; the contract lists it all the same
  if (count && !std::isfinite(vmax * smax)) throw std::invalid_argument("penalty: max(vol) * max(sigma) overflows float32");
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();  // no kernel reads the old contents any more
  if (count == 0) {
    if (!on()) return;
    arena.release();
    buf = nullptr;
    ctr = nullptr;
    sums = SumBuf{};
    n = 0;
    has_forch = has_target = false;
    ++gen;
    return;
  }
  if (!on()) {
    buf = arena.alloc<float>(4 * (size_t)N);
    n = N;
    ++gen;
  }
  if (has_forch != (forch != nullptr) || has_target != (target != nullptr)) ++gen;
  has_forch = forch != nullptr;
  has_target = target != nullptr;
  std::vector<float> h(4 * (size_t)N, 0.0f);  // one upload: sigma | forch | target
  std::memcpy(h.data(), sigma, (size_t)N * sizeof(float));
  if (forch) std::memcpy(h.data() + N, forch, (size_t)N * sizeof(float));
  if (target) std::memcpy(h.data() + 2 * (size_t)N, target, 2 * (size_t)N * sizeof(float));
  CFD_HIP(hipMemcpyAsync(buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, flow.stream));
  flow.sync();  // the staging array is free again
}

void Penalty::set_scale(float s) {
  if (!std::isfinite(s)) throw std::invalid_argument("penalty: target_scale must be finite");
  scale = s;
}

void Penalty::get(const FlowView& flow, float* sigma, float* forch, float* target) const {
  if (!on()) throw std::invalid_argument("penalty: none is set (cfd_set_penalty)");
  if (forch && !has_forch) throw std::invalid_argument("penalty: no forch is set");
  if (target && !has_target) throw std::invalid_argument("penalty: no target is set");
  CFD_HIP(hipSetDevice(flow.device));
  const size_t b = (size_t)n * sizeof(float);
  if (sigma) CFD_HIP(hipMemcpyAsync(sigma, buf, b, hipMemcpyDeviceToHost, flow.stream));
  if (forch) CFD_HIP(hipMemcpyAsync(forch, buf + n, b, hipMemcpyDeviceToHost, flow.stream));
  if (target) CFD_HIP(hipMemcpyAsync(target, buf + 2 * (size_t)n, 2 * b, hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

void Penalty::force(const FlowView& flow, const std::vector<double>& cx, const std::vector<double>& cy, double x0,
                    double y0, const double* box, cfd_penalty_force* out) {
  if (!on()) throw std::invalid_argument("penalty force: no penalty is set (cfd_set_penalty)");
  if (!std::isfinite(x0) || !std::isfinite(y0)) throw std::invalid_argument("penalty force: the centre must be finite");
  if (box)
    for (int k = 0; k < 4; ++k)
      if (std::isnan(box[k])) throw std::invalid_argument("penalty force: a NaN in the box");
  CFD_HIP(hipSetDevice(flow.device));
  if (!ctr) {
    std::vector<double2> h(flow.N);
    for (uint32_t i = 0; i < flow.N; ++i) h[i] = double2{cx[i], cy[i]};
    ctr = arena.upload(h, flow.stream);
    flow.sync();  // h goes out of scope
  }
  PenaltyForceArgs a{};
  a.N = flow.N;
  a.vol = flow.vol;
  a.u = flow.u;
  a.pn = args();
  a.ctr = ctr;
  a.x0 = x0;
  a.y0 = y0;
  a.box_on = box ? 1 : 0;
  if (box) std::memcpy(a.box, box, sizeof(a.box));
  a.out = flow.sums.buf(sums, kPenaltySums, arena);
  launch_penalty_force(a, flow.stream);
  double h[kPenaltySums];
  flow.sum_read(sums, kPenaltySums, h, "penalty force");
  std::memset(out, 0, sizeof(*out));
  out->force[0] = h[0];
  out->force[1] = h[1];
  out->torque = h[2];
  out->power = h[3];
  out->cells = (uint32_t)h[4];
}

}  // namespace cfd2
