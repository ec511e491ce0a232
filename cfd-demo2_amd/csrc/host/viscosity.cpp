// Variable viscosity (include/cfd2_amd.h "Arithmetic of variable viscosity"):
// the per-cell field the VISC forms of prepare, assemble, the flow diagnostics
// and the surface read in place of cfd_constants::viscosity.
#include <cmath>
#include <cstring>

#include "viscosity.hpp"

namespace cfd2 {

void Viscosity::need(const char* what, bool dist, bool ref_mode) {
  if (dist) throw std::invalid_argument(std::string("variable viscosity runs on one GPU only: no ") + what + " on a distributed handle");
  if (ref_mode)
    throw std::invalid_argument(std::string("variable viscosity: no ") + what +
                                " in reference-semantics mode (the racy prepare and the in-place smoother have no such form)");
}

void Viscosity::set(const FlowView& flow, const float* values, uint32_t n) {
  if (n != 0 && n != flow.N)
    throw std::invalid_argument("viscosity field: " + std::to_string(n) + " values for " + std::to_string(flow.N) +
                                " cells (0 clears the field)");
  for (uint32_t i = 0; i < n; ++i)
    if (!std::isfinite(values[i]) || !(values[i] > 0.0f))
      throw std::invalid_argument("viscosity field: cell " + std::to_string(i) + " is not finite and > 0");
  CFD_HIP(hipSetDevice(flow.device));
  flow.sync();  // no kernel reads the old contents any more
  if (n == 0) {
    if (!on()) return;
    arena.release();
    mu = nullptr;
    gdot = nullptr;
    stats = nullptr;
    model = cfd_viscosity_model{};
    ++gen;
    return;
  }
  model = cfd_viscosity_model{};  // setting a field clears a model
  if (!on()) {
    mu = arena.alloc<float>(n);
    ++gen;
  }
  CFD_HIP(hipMemcpyAsync(mu, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice, flow.stream));
  flow.sync();  // the caller's array is free again
}

void Viscosity::get(const FlowView& flow, float* out) const {
  if (!on()) throw std::invalid_argument("viscosity field: none is set (cfd_set_viscosity_field)");
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemcpyAsync(out, mu, (size_t)flow.N * sizeof(float), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

void Viscosity::set_model(const FlowView& flow, const cfd_viscosity_model& m) {
  auto pos = [](float v) { return std::isfinite(v) && v > 0.0f; };
  auto bad = [](const char* what) { throw std::invalid_argument(std::string("viscosity model: ") + what); };
  if (m.kind < 0 || m.kind > 2) bad("kind is 0 (none), 1 (power law) or 2 (Carreau)");
  if (m.kind != 0) {
    if (!std::isfinite(m.n)) bad("n must be finite");
    if (!pos(m.mu_min) || !pos(m.mu_max) || m.mu_min > m.mu_max) bad("0 < mu_min <= mu_max, both finite");
    if (m.kind == 1 && (!pos(m.K) || !pos(m.gamma_min))) bad("power law: K > 0 and gamma_min > 0, both finite");
    if (m.kind == 2 && (!pos(m.mu0) || !std::isfinite(m.mu_inf) || m.mu_inf < 0.0f || !pos(m.lambda)))
      bad("Carreau: mu0 > 0, mu_inf >= 0 and lambda > 0, all finite");
  }
  model = m;
  if (m.kind == 0) return;
  CFD_HIP(hipSetDevice(flow.device));
  if (!on()) {
    flow.sync();
    mu = arena.alloc<float>(flow.N);
    ++gen;
  }
  if (!gdot) {
    gdot = arena.alloc<float>(flow.N);
    stats = arena.alloc<uint32_t>(4);
  }
  evaluate(flow);  // the field is defined from here on
  flow.sync();
}

void Viscosity::evaluate(const FlowView& flow) {
  if (!has_model()) throw std::invalid_argument("viscosity model: none is set (cfd_set_viscosity_model)");
  CFD_HIP(hipSetDevice(flow.device));
  static const uint32_t init[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
  CFD_HIP(hipMemcpyAsync(stats, init, sizeof(init), hipMemcpyHostToDevice, flow.stream));
  ViscosityModelArgs a{};
  a.N = flow.N;
  a.c = flow.constants;
  a.fs = flow.fs;
  a.vol = flow.vol;
  a.u = flow.u;
  a.model = model;
  a.mu = mu;
  a.gdot = gdot;
  a.stats = stats;
  launch_viscosity_model(a, flow.bcv(), flow.stream);
  flow.check_launch("viscosity model");
}

void Viscosity::shear_rate(const FlowView& flow, float* out) const {
  if (!has_model()) throw std::invalid_argument("shear rate: no viscosity model is set (cfd_set_viscosity_model)");
  CFD_HIP(hipSetDevice(flow.device));
  CFD_HIP(hipMemcpyAsync(out, gdot, (size_t)flow.N * sizeof(float), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
}

void Viscosity::stats_get(const FlowView& flow, cfd_viscosity_stats* out) const {
  if (!has_model()) throw std::invalid_argument("viscosity statistics: no viscosity model is set (cfd_set_viscosity_model)");
  CFD_HIP(hipSetDevice(flow.device));
  uint32_t h[4];
  CFD_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, flow.stream));
  flow.sync();
  std::memcpy(&out->mu_min, &h[0], 4);
  std::memcpy(&out->mu_max, &h[1], 4);
  out->clamped_below = h[2];
  out->clamped_above = h[3];
}

}  // namespace cfd2
