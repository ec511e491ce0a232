// Flux and assembly: Rhie-Chow face fluxes and gradients, the coupled system,
// the field update.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"

namespace cfd2 {

namespace {

// Volume penalisation (kernels.hpp PenaltyArgs): pen = vol * s of cell i from
// the iterate uc; the forch test is on a kernel argument, uniform over the launch.
__device__ __forceinline__ float penalty_coeff(const PenaltyArgs& pn, float vol, float2 uc, uint32_t i) {
  float s = pn.sigma[i];
  if (pn.forch) s = s + pn.forch[i] * sqrtf(uc.x * uc.x + uc.y * uc.y);
  return vol * s;
}

// ---------------------------------------------------------------------------
// prepare_coupled.wgsl:63-348 — Rhie-Chow face flux, d_p, Green-Gauss grads.
// Snapshot semantics: reads st (pre-kernel), writes d_p/grad_p to dp_out/gp_out.
// prepare_cell: cell i's face fluxes (stored) and its new d_p, grad_p, grad_u,
// grad_v (returned; k_prepare stores them, k_prepare_ordered after a barrier).
// BCV: the form with prescribed boundary velocities (kernels.hpp BcvArgs): one
// more coalesced 4-byte load per cell, the table only inside a boundary slot's
// branch of a cell that has a row; everything else is the plain form's.
// VISC: the form with a viscosity per cell (kernels.hpp "variable viscosity"):
// one more coalesced 4-byte load per cell and one 4-byte gather per interior
// slot, beside the u[other] gathers; the face viscosity stands where
// c.viscosity stood and nothing else changes.
// PEN: the form with volume penalisation (kernels.hpp PenaltyArgs): after the
// face loop the diagonal takes vol * s, so d_p sees the drag; one to two more
// coalesced 4-byte loads per cell, no gather.
template <bool BCV, bool VISC, bool PEN = false>
__device__ __forceinline__ void prepare_cell(const PrepareArgs& a, const BcvArgs& v, const float* __restrict__ mu,
                                             uint32_t i, float& dp_new, float2& gp_new, float2& gu_new,
                                             float2& gv_new, const PenaltyArgs& pn = PenaltyArgs{}) {
  const uint32_t N = a.N;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const float vol = a.vol[i];
  float diag_coeff = 0.0f;
  float time_coeff = vol * c.density / c.dt;
  if (c.time_scheme == 1u) {
    const float r = c.dt / c.dt_old;
    time_coeff = vol * c.density / c.dt * (1.0f + 2.0f * r) / (1.0f + r);
  }
  diag_coeff += time_coeff;
  const float2 uc = a.st.u[i];
  const float pc = a.st.p[i];
  const float dpc = a.st.dp[i];
  const float2 gpc = a.st.gp[i];
  float gpx = 0.0f, gpy = 0.0f, gux = 0.0f, guy = 0.0f, gvx = 0.0f, gvy = 0.0f;
  const uint32_t nf = fs.nface[i];
  uint32_t brow = 0;
  if constexpr (BCV) brow = v.sel[i];
  float mui = 0.0f;
  if constexpr (VISC) mui = mu[i];
  for (uint32_t k = 0; k < nf; ++k) {
    const size_t e = (size_t)k * N + i;
    const uint32_t meta = fs.meta[e];
    const int32_t other = fs.other[e];
    const uint32_t bt = meta & kMetaBtypeMask;
    const bool own = (meta & kMetaOwner) != 0;
    float mu_f = c.viscosity;  // VISC: the face viscosity, mu[i] on a boundary slot
    if constexpr (VISC) mu_f = mui;
    bool bsel = false;  // BCV: a selected slot, its velocity (sbx, sby)
    float sbx = 0.0f, sby = 0.0f;
    if constexpr (BCV) {
      if (other == kNoCell && brow != 0u) {
        const float4 t = v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
        if (t.z != 0.0f) {
          const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
          const float g = (bt == 1u ? v.inlet_scale : v.wall_scale) * ramp;
          bsel = true;
          sbx = t.x * g;
          sby = t.y * g;
        }
      }
    }
    const float area = fs.area[e];
    const float nx = fs.nx[e], ny = fs.ny[e];  // oriented out of this cell
    // stored face normal, then prepare's geometric re-orientation (wgsl:122-130)
    const float Nx = own ? nx : -nx, Ny = own ? ny : -ny;
    const bool flip = (meta & kMetaFluxFlip) != 0;
    const float nfx = flip ? -Nx : Nx, nfy = flip ? -Ny : Ny;
    float flux = 0.0f;
    float po_other = 0.0f;
    float2 uo = make_float2(0.0f, 0.0f);
    if (other != kNoCell) {
      const float2 u_oth = a.st.u[other];
      const float p_oth = a.st.p[other];
      const float dp_oth = a.st.dp[other];
      const float2 gp_oth = a.st.gp[other];
      if constexpr (VISC) mu_f = 0.5f * (mui + mu[other]);
      uo = u_oth;
      po_other = p_oth;
      const float2 uow = own ? uc : u_oth, ung = own ? u_oth : uc;
      const float pow_ = own ? pc : p_oth, png = own ? p_oth : pc;
      const float dpow = own ? dpc : dp_oth, dpng = own ? dp_oth : dpc;
      const float2 gpow = own ? gpc : gp_oth, gpng = own ? gp_oth : gpc;
      const float lambda = fs.lam_f[e];
      const float ufx = lambda * uow.x + (1.0f - lambda) * ung.x;
      const float ufy = lambda * uow.y + (1.0f - lambda) * ung.y;
      const float dp_face = lambda * dpow + (1.0f - lambda) * dpng;
      const float gfx = lambda * gpow.x + (1.0f - lambda) * gpng.x;
      const float gfy = lambda * gpow.y + (1.0f - lambda) * gpng.y;
      const float dist = fs.dist_a[e];
      const float grad_p_n = gfx * nfx + gfy * nfy;
      const float p_grad_f = (png - pow_) / dist;
      const float rc_term = dp_face * area * (grad_p_n - p_grad_f);
      const float u_n = ufx * nfx + ufy * nfy;
      flux = c.density * (u_n * area + rc_term);
    } else if (bt == 1u) {
      const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
      float ubx = c.inlet_velocity * ramp, uby = 0.0f;
      if constexpr (BCV) {
        if (bsel) {
          ubx = sbx;
          uby = sby;
        }
      }
      flux = c.density * (ubx * nfx + uby * nfy) * area;
    } else if (bt == 2u) {
      const float u_n = uc.x * nfx + uc.y * nfy;  // boundary faces are owned by this cell
      const float raw = c.density * u_n * area;
      flux = fmaxf(0.0f, raw);
    }
    const float flux_out = own ? flux : -flux;
    a.flux_s[e] = flux_out;
    const float diff_coeff = mu_f * area / fs.dist_e[e];
    const float conv_diag = flux_out > 0.0f ? flux_out : 0.0f;
    if (other != kNoCell) {
      diag_coeff += diff_coeff + conv_diag;
    } else if (bt == 1u || bt == 3u) {
      diag_coeff += diff_coeff;
      if (flux_out > 0.0f) diag_coeff += flux_out;
    } else if (bt == 2u) {
      if (flux_out > 0.0f) diag_coeff += flux_out;
    }
    float vfp, vfu, vfv;  // k_flow_diag (diagnostics.hip) carries a copy of the vfu / vfv branch
    if (other != kNoCell) {
      const float lp = fs.lam_s[e];
      vfp = lp * pc + (1.0f - lp) * po_other;
      if ((meta & kMetaDegen) == 0) {
        vfu = lp * uc.x + (1.0f - lp) * uo.x;
        vfv = lp * uc.y + (1.0f - lp) * uo.y;
      } else {
        vfu = 0.5f * (uc.x + uo.x);
        vfv = 0.5f * (uc.y + uo.y);
      }
    } else {
      vfp = (bt == 2u) ? 0.0f : pc;
      if (bt == 1u) {
        const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
        vfu = c.inlet_velocity * ramp;
        vfv = 0.0f;
      } else if (bt == 3u) {
        vfu = 0.0f;
        vfv = 0.0f;
      } else {
        vfu = uc.x;
        vfv = uc.y;
      }
      if constexpr (BCV) {
        if (bsel) {
          vfu = sbx;
          vfv = sby;
        }
      }
    }
    gpx += vfp * nx * area;
    gpy += vfp * ny * area;
    gux += vfu * nx * area;
    guy += vfu * ny * area;
    gvx += vfv * nx * area;
    gvy += vfv * ny * area;
  }
  if constexpr (PEN) diag_coeff += penalty_coeff(pn, vol, uc, i);
  dp_new = (fabsf(diag_coeff) > 1e-20f) ? vol / diag_coeff : 0.0f;
  gp_new = make_float2(gpx / vol, gpy / vol);
  gu_new = make_float2(gux / vol, guy / vol);
  gv_new = make_float2(gvx / vol, gvy / vol);
}
__global__ void __launch_bounds__(kBlock) k_prepare(PrepareArgs a) {
  const uint32_t i = row_id();
  if (i >= a.N) return;
  float dp;
  float2 gp, gu, gv;
  prepare_cell<false, false>(a, BcvArgs{}, nullptr, i, dp, gp, gu, gv);
  a.dp_out[i] = dp;
  a.gp_out[i] = gp;
  a.grad_u[i] = gu;
  a.grad_v[i] = gv;
}
__global__ void __launch_bounds__(kBlock) k_prepare_bcv(PrepareArgs a, BcvArgs v) {
  const uint32_t i = row_id();
  if (i >= a.N) return;
  float dp;
  float2 gp, gu, gv;
  prepare_cell<true, false>(a, v, nullptr, i, dp, gp, gu, gv);
  a.dp_out[i] = dp;
  a.gp_out[i] = gp;
  a.grad_u[i] = gu;
  a.grad_v[i] = gv;
}
__global__ void __launch_bounds__(kBlock) k_prepare_visc(PrepareArgs a, const float* __restrict__ mu) {
  const uint32_t i = row_id();
  if (i >= a.N) return;
  float dp;
  float2 gp, gu, gv;
  prepare_cell<false, true>(a, BcvArgs{}, mu, i, dp, gp, gu, gv);
  a.dp_out[i] = dp;
  a.gp_out[i] = gp;
  a.grad_u[i] = gu;
  a.grad_v[i] = gv;
}
__global__ void __launch_bounds__(kBlock) k_prepare_bcv_visc(PrepareArgs a, BcvArgs v, const float* __restrict__ mu) {
  const uint32_t i = row_id();
  if (i >= a.N) return;
  float dp;
  float2 gp, gu, gv;
  prepare_cell<true, true>(a, v, mu, i, dp, gp, gu, gv);
  a.dp_out[i] = dp;
  a.gp_out[i] = gp;
  a.grad_u[i] = gu;
  a.grad_v[i] = gv;
}
// the PEN forms: every argument struct, the unused ones empty
template <bool BCV, bool VISC>
__global__ void __launch_bounds__(kBlock) k_prepare_pen(PrepareArgs a, BcvArgs v, const float* __restrict__ mu,
                                                        PenaltyArgs pn) {
  const uint32_t i = row_id();
  if (i >= a.N) return;
  float dp;
  float2 gp, gu, gv;
  prepare_cell<BCV, VISC, true>(a, v, mu, i, dp, gp, gu, gv, pn);
  a.dp_out[i] = dp;
  a.gp_out[i] = gp;
  a.grad_u[i] = gu;
  a.grad_v[i] = gv;
}
// The reference's RACY prepare (prepare_coupled.wgsl:140-143 vs :328-337)
// under one legal schedule (test mode, Solver::ref_racy; oracle
// kSemRacyPrepare): the 64-cell workgroups one after another, d_p / grad_p
// written in place (dp_out == st.dp, gp_out == st.gp), every cell of a
// workgroup reading before any writes -- later workgroups read the new values.
__global__ void __launch_bounds__(64) k_prepare_ordered(PrepareArgs a) {
  for (uint32_t b0 = 0; b0 < a.N; b0 += 64) {
    const uint32_t i = b0 + threadIdx.x;
    float dp = 0.0f;
    float2 gp = make_float2(0.0f, 0.0f), gu = gp, gv = gp;
    if (i < a.N) prepare_cell<false, false>(a, BcvArgs{}, nullptr, i, dp, gp, gu, gv);
    __syncthreads();  // the workgroup's reads complete
    if (i < a.N) {
      a.dp_out[i] = dp;
      a.gp_out[i] = gp;
      a.grad_u[i] = gu;
      a.grad_v[i] = gv;
    }
    __syncthreads();  // visible to the next workgroup
  }
}
// the assembly reads fluxes[face] as the OWNER stored it (coupled_assembly_
// merged.wgsl:153): a non-owner slot takes -(owner's flux) -- the same bits as
// its own computation under snapshot reads, not under the racy ones
__global__ void __launch_bounds__(kBlock) k_flux_mirror(float* flux_s, const int32_t* mirror, uint32_t S) {
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S) return;
  const int32_t m = mirror[e];
  if (m >= 0) flux_s[e] = -flux_s[m];  // owner slots (m < 0) are only read
}

// coupled_assembly_merged.wgsl:70-463.  BUOY: the form with the Boussinesq
// source (kernels.hpp BuoyancyArgs): one more coalesced 4-byte load per driving
// field, after the face loop; everything else is the plain form's.  The
// arguments come by value: by reference the compiler schedules the QUICK
// branch's loads differently, and k_assemble is to stay the code it was.
// BCV: the form with prescribed boundary velocities (kernels.hpp BcvArgs), as in
// prepare_cell: nothing is added to an interior slot.
// VISC: the form with a viscosity per cell, as in prepare_cell, with this
// kernel's own distance (dist_a); the gather sits beside dp[other].
// PEN: the form with volume penalisation (kernels.hpp PenaltyArgs): after the
// face loop and the BUOY block the diagonal takes vol * s and, with a target,
// the right-hand side vol * s * (target_scale * target); no off-diagonal changes.
template <bool BUOY, bool BCV, bool VISC, bool PEN = false>
__device__ __forceinline__ void assemble_cell(const AssembleArgs a, const BuoyancyArgs b, const BcvArgs v,
                                              const float* __restrict__ mu, const PenaltyArgs pn = PenaltyArgs{}) {
  const uint32_t i = row_id();
  const uint32_t N = a.N;
  if (i >= N) return;
  const cfd_constants c = a.c;
  const FaceSlots fs = a.fs;
  const float vol = a.vol[i];
  float diag_uv = 0.0f;  // diag_u == diag_v (identical update sequence)
  float sdup = 0.0f, sdvp = 0.0f, sdpu = 0.0f, sdpv = 0.0f, sdpp = 0.0f;
  float rhs_u = 0.0f, rhs_v = 0.0f, rhs_p = 0.0f, sdiag = 0.0f;
  const float2 un = a.u_old[i];
  float coeff_time = vol * c.density / c.dt;
  float rtu = coeff_time * un.x, rtv = coeff_time * un.y;
  if (c.time_scheme == 1u) {
    const float dt = c.dt, dt_old = c.dt_old;
    const float r = dt / dt_old;
    const float2 unm1 = a.u_old_old[i];
    coeff_time = vol * c.density / dt * (1.0f + 2.0f * r) / (1.0f + r);
    const float fn = (1.0f + r);
    const float fnm1 = (r * r) / (1.0f + r);
    rtu = (vol * c.density / dt) * (fn * un.x - fnm1 * unm1.x);
    rtv = (vol * c.density / dt) * (fn * un.y - fnm1 * unm1.y);
  }
  diag_uv += coeff_time;
  rhs_u += rtu;
  rhs_v += rtv;
  const float dpc = a.st.dp[i];
  const float2 uc = a.st.u[i];
  const uint32_t nf = fs.nface[i];
  uint32_t brow = 0;
  if constexpr (BCV) brow = v.sel[i];
  float mui = 0.0f;
  if constexpr (VISC) mui = mu[i];
  for (uint32_t k = 0; k < nf; ++k) {
    const size_t e = (size_t)k * N + i;
    const uint32_t meta = fs.meta[e];
    const int32_t other = fs.other[e];
    const uint32_t bt = meta & kMetaBtypeMask;
    const float area = fs.area[e];
    const float nx = fs.nx[e], ny = fs.ny[e];
    const float flux = a.flux_s[e];
    const float dist = fs.dist_a[e];
    float mu_f = c.viscosity;  // VISC: the face viscosity, mu[i] on a boundary slot
    if constexpr (VISC) mu_f = other != kNoCell ? 0.5f * (mui + mu[other]) : mui;
    const float diff_coeff = mu_f * area / dist;
    const float conv_diag = flux > 0.0f ? flux : 0.0f;
    const float conv_off = flux > 0.0f ? 0.0f : flux;
    if (other != kNoCell) {
      const uint32_t rank = (meta >> kMetaRankShift) & 0xFFu;
      const float dp_other = a.st.dp[other];
      const float coeff = -diff_coeff + conv_off;
      diag_uv += diff_coeff + conv_diag;
      if (c.scheme != 0u) {
        const float2 uo = a.st.u[other];
        float pu_u = uc.x, pu_v = uc.y;
        if (flux < 0.0f) {
          pu_u = uo.x;
          pu_v = uo.y;
        }
        float ph_u = pu_u, ph_v = pu_v;
        if (c.scheme == 1u) {
          if (flux > 0.0f) {
            const float2 gu = a.grad_u[i], gv = a.grad_v[i];
            const float rx = fs.rx[e], ry = fs.ry[e];
            ph_u = uc.x + (gu.x * rx + gu.y * ry);
            ph_v = uc.y + (gv.x * rx + gv.y * ry);
          } else {
            const float2 gu = a.grad_u[other], gv = a.grad_v[other];
            const float rx = fs.rox[e], ry = fs.roy[e];
            ph_u = uo.x + (gu.x * rx + gu.y * ry);
            ph_v = uo.y + (gv.x * rx + gv.y * ry);
          }
        } else if (c.scheme == 2u) {
          if (flux > 0.0f) {
            const float2 gu = a.grad_u[i], gv = a.grad_v[i];
            const float dx = fs.dvx[e], dy = fs.dvy[e];
            const float gtu = gu.x * dx + gu.y * dy, gtv = gv.x * dx + gv.y * dy;
            ph_u = 0.625f * uc.x + 0.375f * uo.x + 0.125f * gtu;
            ph_v = 0.625f * uc.y + 0.375f * uo.y + 0.125f * gtv;
          } else {
            const float2 gu = a.grad_u[other], gv = a.grad_v[other];
            const float dx = -fs.dvx[e], dy = -fs.dvy[e];  // center - other_center
            const float gtu = gu.x * dx + gu.y * dy, gtv = gv.x * dx + gv.y * dy;
            ph_u = 0.625f * uo.x + 0.375f * uc.x + 0.125f * gtu;
            ph_v = 0.625f * uo.y + 0.375f * uc.y + 0.125f * gtv;
          }
        }
        rhs_u -= flux * (ph_u - pu_u);
        rhs_v -= flux * (ph_v - pu_v);
      }
      const float lambda = fs.lam_s[e];
      const float oml = 1.0f - lambda;
      const float pgx = area * nx, pgy = area * ny;
      sdup += lambda * pgx;
      sdvp += lambda * pgy;
      const float dcx = nx * area, dcy = ny * area;
      sdpu += lambda * dcx;
      sdpv += lambda * dcy;
      const float dp_f = lambda * dpc + (1.0f - lambda) * dp_other;
      const float lapl = dp_f * area / dist;
      sdpp += lapl;
      const float scoeff = c.density * dp_f * area / dist;
      sdiag += scoeff;
      const size_t cslot = (size_t)((meta >> kMetaTSlotShift) & 0xFFu) * a.ld + i;
      a.cval_a[cslot] = make_float2(coeff, -lapl);
      a.cval_g[cslot] = make_float2(oml * pgx, oml * pgy);
      a.sval[(size_t)rank * a.ld + i] = -scoeff;
    } else if (bt == 1u) {
      const float ramp = wsmoothstep(0.0f, c.ramp_time, c.time);
      float ubx = c.inlet_velocity * ramp, uby = 0.0f;
      if constexpr (BCV) {
        if (brow != 0u) {
          const float4 t = v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
          if (t.z != 0.0f) {
            const float g = v.inlet_scale * ramp;
            ubx = t.x * g;
            uby = t.y * g;
          }
        }
      }
      diag_uv += diff_coeff;
      rhs_u += diff_coeff * ubx;
      rhs_v += diff_coeff * uby;
      if (flux > 0.0f) {
        diag_uv += flux;
      } else {
        rhs_u -= flux * ubx;
        rhs_v -= flux * uby;
      }
      sdup += area * nx;
      sdvp += area * ny;
      const float flux_bc = (ubx * nx + uby * ny) * area;
      rhs_p -= flux_bc;
    } else if (bt == 3u) {
      diag_uv += diff_coeff;
      sdup += area * nx;
      sdvp += area * ny;
      if constexpr (BCV) {
        if (brow != 0u) {
          const float4 t = v.tab[(size_t)(brow - 1u) * (uint32_t)fs.wf + k];
          if (t.z != 0.0f) {
            const float g = v.wall_scale * wsmoothstep(0.0f, c.ramp_time, c.time);
            rhs_u += diff_coeff * (t.x * g);
            rhs_v += diff_coeff * (t.y * g);
          }
        }
      }
    } else if (bt == 2u) {
      if (flux > 0.0f) diag_uv += flux;
      sdpu += nx * area;
      sdpv += ny * area;
      const float lapl = dpc * area / dist;
      sdpp += lapl;
      const float scoeff = c.density * dpc * area / dist;
      sdiag += scoeff;
    }
  }
  if constexpr (BUOY) {
    const float vr = vol * c.density;
#pragma unroll
    for (int f = 0; f < kMaxBuoyancyFields; ++f) {  // unrolled: every entry a fixed kernel-argument offset
      if (f < b.n) {
        const float d = b.f[f].phi[i] - b.f[f].ref;
        const float fb = vr * (b.f[f].beta * d);
        rhs_u = rhs_u - fb * b.gx;
        rhs_v = rhs_v - fb * b.gy;
      }
    }
  }
  if constexpr (PEN) {
    const float pen = penalty_coeff(pn, vol, uc, i);
    diag_uv += pen;
    if (pn.target) {
      const float2 ut = pn.target[i];
      rhs_u += pen * (pn.target_scale * ut.x);
      rhs_v += pen * (pn.target_scale * ut.y);
    }
  }
  const size_t cdslot = (size_t)a.cslot_diag[i] * a.ld + i;
  a.cval_a[cdslot] = make_float2(diag_uv, 0.0f + sdpp);
  a.cval_g[cdslot] = make_float2(sdup, sdvp);
  a.cdiag2[i] = make_float2(sdpu, sdpv);
  a.sval[(size_t)a.srank_diag[i] * a.ld + i] = sdiag;
  a.rhs[3 * (size_t)i + 0] = rhs_u;
  a.rhs[3 * (size_t)i + 1] = rhs_v;
  a.rhs[3 * (size_t)i + 2] = rhs_p;
  a.dinv_uv[i] = safe_inverse(diag_uv);
  a.dinv_p[i] = safe_inverse(sdiag);
}
__global__ void __launch_bounds__(kBlock) k_assemble(AssembleArgs a) {
  assemble_cell<false, false, false>(a, BuoyancyArgs{}, BcvArgs{}, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_assemble_buoyant(AssembleArgs a, BuoyancyArgs b) {
  assemble_cell<true, false, false>(a, b, BcvArgs{}, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_assemble_bcv(AssembleArgs a, BcvArgs v) {
  assemble_cell<false, true, false>(a, BuoyancyArgs{}, v, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_assemble_buoyant_bcv(AssembleArgs a, BuoyancyArgs b, BcvArgs v) {
  assemble_cell<true, true, false>(a, b, v, nullptr);
}
__global__ void __launch_bounds__(kBlock) k_assemble_visc(AssembleArgs a, const float* __restrict__ mu) {
  assemble_cell<false, false, true>(a, BuoyancyArgs{}, BcvArgs{}, mu);
}
__global__ void __launch_bounds__(kBlock) k_assemble_buoyant_visc(AssembleArgs a, BuoyancyArgs b,
                                                                  const float* __restrict__ mu) {
  assemble_cell<true, false, true>(a, b, BcvArgs{}, mu);
}
__global__ void __launch_bounds__(kBlock) k_assemble_bcv_visc(AssembleArgs a, BcvArgs v, const float* __restrict__ mu) {
  assemble_cell<false, true, true>(a, BuoyancyArgs{}, v, mu);
}
__global__ void __launch_bounds__(kBlock) k_assemble_buoyant_bcv_visc(AssembleArgs a, BuoyancyArgs b, BcvArgs v,
                                                                      const float* __restrict__ mu) {
  assemble_cell<true, true, true>(a, b, v, mu);
}
template <bool BUOY, bool BCV, bool VISC>
__global__ void __launch_bounds__(kBlock) k_assemble_pen(AssembleArgs a, BuoyancyArgs b, BcvArgs v,
                                                         const float* __restrict__ mu, PenaltyArgs pn) {
  assemble_cell<BUOY, BCV, VISC, true>(a, b, v, mu, pn);
}

// update_fields_from_coupled.wgsl:45-98.  The reference folds max|du|, max|dp|
// with one atomicMax per workgroup into a single word; here each block writes
// the max of its bit patterns (order-independent) and k_maxdiff_final folds
// them, avoiding ~40k same-address atomics per call.
__global__ void __launch_bounds__(kBlock) k_update_fields(uint32_t N, float alpha_u, float alpha_p,
                                                          const float* __restrict__ x, float2* u,
                                                          float* p, uint32_t* blockmax) {
  __shared__ uint32_t su[4], sp[4];
  const uint32_t lb = xcd_block();
  const uint32_t i = lb * kBlock + threadIdx.x;
  uint32_t bu = 0, bp = 0;
  if (i < N) {
    const float un = x[3 * (size_t)i], vn = x[3 * (size_t)i + 1], pn = x[3 * (size_t)i + 2];
    const float2 uo = u[i];
    const float po = p[i];
    const float ux = uo.x + alpha_u * (un - uo.x);
    const float uy = uo.y + alpha_u * (vn - uo.y);
    const float pu = po + alpha_p * (pn - po);
    u[i] = make_float2(ux, uy);
    p[i] = pu;
    const float du = fmaxf(fabsf(ux - uo.x), fabsf(uy - uo.y));
    const float dp = fabsf(pu - po);
    bu = __float_as_uint(du);
    bp = __float_as_uint(dp);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    bu = max(bu, (uint32_t)__shfl_xor((int)bu, o));
    bp = max(bp, (uint32_t)__shfl_xor((int)bp, o));
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    su[wv] = bu;
    sp[wv] = bp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blockmax[2 * lb] = max(max(su[0], su[1]), max(su[2], su[3]));
    blockmax[2 * lb + 1] = max(max(sp[0], sp[1]), max(sp[2], sp[3]));
  }
}

__global__ void __launch_bounds__(kBlock) k_maxdiff_final(const uint32_t* __restrict__ blockmax,
                                                          uint32_t nb, uint32_t* maxbits, uint32_t* host_out) {
  __shared__ uint32_t su[4], sp[4];
  uint32_t bu = 0, bp = 0;
  for (uint32_t q = threadIdx.x; q < nb; q += kBlock) {
    const uint2 v = *reinterpret_cast<const uint2*>(blockmax + 2 * (size_t)q);
    bu = max(bu, v.x);
    bp = max(bp, v.y);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    bu = max(bu, (uint32_t)__shfl_xor((int)bu, o));
    bp = max(bp, (uint32_t)__shfl_xor((int)bp, o));
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    su[wv] = bu;
    sp[wv] = bp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    maxbits[0] = max(max(su[0], su[1]), max(su[2], su[3]));
    maxbits[1] = max(max(sp[0], sp[1]), max(sp[2], sp[3]));
    if (host_out) {  // mapped pinned host memory: the host's lagged read needs no copy
      host_out[0] = maxbits[0];
      host_out[1] = maxbits[1];
    }
  }
}

}  // namespace

void launch_prepare(const PrepareArgs& a, hipStream_t s) {
  if (a.N) hipLaunchKernelGGL(k_prepare, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a);
}
void launch_prepare_ordered(const PrepareArgs& a, const int32_t* mirror, uint32_t slots, hipStream_t s) {
  if (!a.N) return;
  hipLaunchKernelGGL(k_prepare_ordered, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_flux_mirror, dim3((slots + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a.flux_s, mirror, slots);
}
void launch_assemble(const AssembleArgs& a, hipStream_t s) {
  if (a.N) hipLaunchKernelGGL(k_assemble, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a);
}
void launch_assemble_buoyant(const AssembleArgs& a, const BuoyancyArgs& b, hipStream_t s) {
  if (a.N) hipLaunchKernelGGL(k_assemble_buoyant, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, b);
}
void launch_prepare_bcv(const PrepareArgs& a, const BcvArgs& v, hipStream_t s) {
  if (a.N) hipLaunchKernelGGL(k_prepare_bcv, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, v);
}
void launch_assemble_bcv(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs& v, hipStream_t s) {
  if (!a.N) return;
  if (buoy)
    hipLaunchKernelGGL(k_assemble_buoyant_bcv, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, *buoy, v);
  else
    hipLaunchKernelGGL(k_assemble_bcv, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, v);
}
void launch_prepare_visc(const PrepareArgs& a, const BcvArgs* v, const float* mu, hipStream_t s) {
  if (!a.N) return;
  if (v)
    hipLaunchKernelGGL(k_prepare_bcv_visc, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, *v, mu);
  else
    hipLaunchKernelGGL(k_prepare_visc, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, mu);
}
void launch_assemble_visc(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs* v, const float* mu,
                          hipStream_t s) {
  if (!a.N) return;
  const dim3 g(grid_for(a.N)), b(kBlock);
  if (buoy && v)
    hipLaunchKernelGGL(k_assemble_buoyant_bcv_visc, g, b, 0, s, a, *buoy, *v, mu);
  else if (v)
    hipLaunchKernelGGL(k_assemble_bcv_visc, g, b, 0, s, a, *v, mu);
  else if (buoy)
    hipLaunchKernelGGL(k_assemble_buoyant_visc, g, b, 0, s, a, *buoy, mu);
  else
    hipLaunchKernelGGL(k_assemble_visc, g, b, 0, s, a, mu);
}
void launch_prepare_pen(const PrepareArgs& a, const BcvArgs* v, const float* mu, const PenaltyArgs& pn, hipStream_t s) {
  if (!a.N) return;
  const BcvArgs vv = v ? *v : BcvArgs{};
  auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, vv, mu, pn); };
  if (v && mu)
    go(k_prepare_pen<true, true>);
  else if (v)
    go(k_prepare_pen<true, false>);
  else if (mu)
    go(k_prepare_pen<false, true>);
  else
    go(k_prepare_pen<false, false>);
}
void launch_assemble_pen(const AssembleArgs& a, const BuoyancyArgs* buoy, const BcvArgs* v, const float* mu,
                         const PenaltyArgs& pn, hipStream_t s) {
  if (!a.N) return;
  const BuoyancyArgs bb = buoy ? *buoy : BuoyancyArgs{};
  const BcvArgs vv = v ? *v : BcvArgs{};
  auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(grid_for(a.N)), dim3(kBlock), 0, s, a, bb, vv, mu, pn); };
  auto visc = [&](auto with, auto without) { mu ? go(with) : go(without); };
  if (buoy && v)
    visc(k_assemble_pen<true, true, true>, k_assemble_pen<true, true, false>);
  else if (buoy)
    visc(k_assemble_pen<true, false, true>, k_assemble_pen<true, false, false>);
  else if (v)
    visc(k_assemble_pen<false, true, true>, k_assemble_pen<false, true, false>);
  else
    visc(k_assemble_pen<false, false, true>, k_assemble_pen<false, false, false>);
}
void launch_update_fields(uint32_t N, float au, float ap, const float* x, float2* u, float* p,
                          uint32_t* blockmax, uint32_t* maxbits, uint32_t* host_out, hipStream_t s) {
  if (!N) return;
  const unsigned nb = grid_for(N);
  hipLaunchKernelGGL(k_update_fields, dim3(nb), dim3(kBlock), 0, s, N, au, ap, x, u, p, blockmax);
  hipLaunchKernelGGL(k_maxdiff_final, dim3(1), dim3(kBlock), 0, s, blockmax, nb, maxbits, host_out);
}

}  // namespace cfd2
