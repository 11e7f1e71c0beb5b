// predict_sum's read-out (src/api.jl:898-936 on top of predict_mvn_sum, 978-1034), on the device marginals of a chunk of particles
// before anything goes back to the host: predict_mvn_sum's raw-space transform for a linear y_transform (Transforms.jl:44-49),
//   mu_raw = (mu - b) / a  (+ b / a on the F_1 rows: the intercept counted once),   var_raw = (1 / a^2) var,
// and the marginal quantiles of src/GP.jl:1006-1012, quantile(Normal(mu_raw, sqrt(var_raw)), q) = fma(sigma, ndtri(q), mu_raw) with
// ndtri(q) formed on the host (csrc/agp_ndtri.hpp).  One thread per (particle, joint row); each row is its own: a particle's results
// depend on its own marginals alone.  A row whose raw variance is negative or NaN, or whose raw mean is not finite, marks its
// particle: bad[p] = min(row + 1) (atomicMin, order-free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "agp_args.hpp"

namespace agp {

// (SumReadArgs: agp_args.hpp)

__global__ void k_sum_readout(SumReadArgs a) {
  const int p = blockIdx.y;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.m) return;
  const long long o = (long long)p * a.m + g;
  double mr = (a.mean[o] - a.intercept) / a.slope;
  if (g < a.p_rows) mr = mr + a.shift;
  const double vr = a.ivar * a.var[o];
  a.mean[o] = mr;
  const bool ok = isfinite(mr) && vr >= 0.0;
  if (!ok) atomicMin(a.bad + p, g + 1);
  const double sd = ok ? sqrt(vr) : __builtin_nan("");
  double* xo = a.x + o * a.nq;
  for (int k = 0; k < a.nq; ++k) xo[k] = fma(sd, a.z[k], mr);
}

}  // namespace agp
