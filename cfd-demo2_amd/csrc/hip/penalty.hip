// Volume penalisation, the diagnostic (kernels.hpp PenaltyForceArgs; include/
// cfd2_amd.h "Arithmetic of volume penalisation"): k_penalty_force, one
// read-only pass over the cells of the current state, five f64 sums over the
// shared cell-sum skeleton (reduce_dev.hpp), so the bits do not depend on the
// scheduling.  Per cell 4 B (vol), 8 B (u), 16 B (the f64 centre), 4 B (sigma)
// and 4 B / 8 B more with forch / target, all coalesced.
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"
#include "reduce_dev.hpp"

namespace cfd2 {

namespace {

__global__ void __launch_bounds__(kBlock) k_penalty_force(PenaltyForceArgs a) {
  __shared__ double lsum[kPenaltySums][4][4];  // [sum][chunk q][quarter w]
  const uint32_t N = a.N;
  const uint32_t lb = xcd_block();
  const double scale = (double)a.pn.target_scale;
  sum_accumulate<kPenaltySums>(lsum, N, lb, [&](uint32_t i, double* t) {
    const double2 ctr = a.ctr[i];
    if (a.box_on && !(ctr.x >= a.box[0] && ctr.x <= a.box[2] && ctr.y >= a.box[1] && ctr.y <= a.box[3])) return;
    const float2 uc = a.u[i];
    const double ux = (double)uc.x, uy = (double)uc.y;
    double s = (double)a.pn.sigma[i];
    if (a.pn.forch) s = s + (double)a.pn.forch[i] * sqrt(ux * ux + uy * uy);
    const double m = (double)a.vol[i] * s;
    double tx = 0.0, ty = 0.0;
    if (a.pn.target) {
      const float2 ut = a.pn.target[i];
      tx = scale * (double)ut.x;
      ty = scale * (double)ut.y;
    }
    const double fx = m * (ux - tx), fy = m * (uy - ty);
    const double rx = ctr.x - a.x0, ry = ctr.y - a.y0;
    t[0] = fx;
    t[1] = fy;
    t[2] = rx * fy - ry * fx;
    t[3] = fx * tx + fy * ty;
    t[4] = s > 0.0 ? 1.0 : 0.0;
  });
  __syncthreads();
  sum_store<kPenaltySums>(lsum, a.out, N, lb);
}

}  // namespace

void launch_penalty_force(const PenaltyForceArgs& a, hipStream_t s) {
  const uint32_t nb = red_blocks(a.N);
  if (nb) hipLaunchKernelGGL(k_penalty_force, dim3(nb), dim3(kBlock), 0, s, a);
}

}  // namespace cfd2
