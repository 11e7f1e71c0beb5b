// Moments of a mixture of Gaussians (Distributions.mean / var / cov of the MixtureModel predict_mvn returns, src/api.jl:497-522)
// reduced over the particles on the device, chunk by chunk of the predictive pass.  With weights w_p (sum 1) and components of mean
// e_p and covariance C_p:
//     mean = sum w_p e_p,      cov = sum w_p (C_p + (e_p - mean)(e_p - mean)'),      var = diag(cov).
// The sums run about a pivot s (the mean of the first component of positive weight: inside the range of the means, coordinate by
// coordinate), never about 0 — sum w (C + e e') - mean mean' cancels catastrophically when the means share an offset:
//     S1 = sum w_p (e_p - s),   S2 = sum w_p (C_p + (e_p - s)(e_p - s)'),   mean = s + S1,   cov = S2 - S1 S1'.
// Every element is summed sequentially in the pass's particle order and continues from the value the previous chunk left (no
// atomics, no tree): the bits do not depend on how the pass is chunked.  A component of weight 0 is skipped, whatever it holds.
// Components: the raw-space transform of predict_mvn first, mu_r = (mu - b) / a, C_r = C / a^2; then
//   space 0   e = mu_r,                         C_p = C_r
//   space 1   e_i = exp(mu_r,i + C_r,ii / 2),   C_p,ij = e_i e_j expm1(C_r,ij)      (MvLogNormal(N(mu_r, C_r)); Transforms.jl:87-91)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "agp_args.hpp"
#include "agp_math.hpp"

namespace agp {

constexpr int MIXMOM_TI = 64, MIXMOM_TJ = 4;      // k_mixmom_cov's workgroup: 64 consecutive rows i (one wave) of 4 columns j

// exp as the log-normal components call it (exp_f's domain ends where exp overflows: the reference's Inf)
__device__ __forceinline__ double mixmom_exp(double x) { return x > 709.782712893384 ? __builtin_inf() : fm::exp_f(x); }

// mean (output space) and variance of component p at point i
__device__ __forceinline__ void mixmom_component(const MixMomArgs& a, int p, int i, double* e, double* d) {
  const double mr = (a.mean[(long long)p * a.m + i] - a.intercept) / a.slope;
  const double vr = a.ivar * a.var[(long long)p * a.v_pstride + (long long)i * a.v_istride];
  if (a.space == 0) { *e = mr; *d = vr; return; }
  const double ex = mixmom_exp(fma(0.5, vr, mr));
  *e = ex;
  *d = ex * ex * expm1(vr);
}

// S1 and the diagonal of S2, one thread per query point (coalesced along i: mean / var are [Pc][m]); writes the chunk's e
__global__ void k_mixmom_marginal(MixMomArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  double s, s1 = 0.0, s2 = 0.0, e, d;
  if (a.pivot >= 0) {
    mixmom_component(a, a.pivot, i, &s, &d);
    a.s[i] = s;
  } else {
    s = a.s[i]; s1 = a.s1[i]; s2 = a.s2d[i];
  }
  for (int p = 0; p < a.Pc; ++p) {
    const double w = a.w[p];
    if (w == 0.0) continue;
    mixmom_component(a, p, i, &e, &d);
    a.e[(long long)p * a.m + i] = e;
    const double r = e - s;
    s1 = fma(w, r, s1);
    s2 = fma(w, fma(r, r, d), s2);
  }
  a.s1[i] = s1; a.s2d[i] = s2;
}

// lower triangle of S2, one thread per element (i, j), i >= j: each element of C_p is read once, consecutive lanes consecutive i
__global__ __launch_bounds__(MIXMOM_TI * MIXMOM_TJ) void k_mixmom_cov(MixMomArgs a) {
  if ((int)blockIdx.x * MIXMOM_TI + MIXMOM_TI - 1 < (int)blockIdx.y * MIXMOM_TJ) return;      // wholly above the diagonal
  const int i = blockIdx.x * MIXMOM_TI + threadIdx.x, j = blockIdx.y * MIXMOM_TJ + threadIdx.y;
  if (i >= a.m || j >= a.m || i < j) return;
  const long long mm = (long long)a.m * a.m, idx = (long long)j * a.m + i;
  const double si = a.s[i], sj = a.s[j];
  double acc = a.pivot >= 0 ? 0.0 : a.acc[idx];
  for (int p = 0; p < a.Pc; ++p) {
    const double w = a.w[p];
    if (w == 0.0) continue;
    const double ei = a.e[(long long)p * a.m + i], ej = a.e[(long long)p * a.m + j];
    double c = a.ivar * a.cov[(long long)p * mm + idx];
    if (a.space != 0) c = ei * ej * expm1(c);
    acc = fma(w, fma(ei - si, ej - sj, c), acc);
  }
  a.acc[idx] = acc;
}

// marginal pass: mean = s + S1, var = S2_ii - S1_i^2
__global__ void k_mixmom_finish_marginal(MixMomArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  const double s1 = a.s1[i];
  a.out_mean[i] = a.s[i] + s1;
  a.out_var[i] = fma(-s1, s1, a.s2d[i]);
}

// covariance pass: cov = S2 - S1 S1' mirrored over the diagonal, var = its diagonal (the same bits), mean = s + S1
__global__ __launch_bounds__(MIXMOM_TI * MIXMOM_TJ) void k_mixmom_finish_cov(MixMomArgs a) {
  if ((int)blockIdx.x * MIXMOM_TI + MIXMOM_TI - 1 < (int)blockIdx.y * MIXMOM_TJ) return;
  const int i = blockIdx.x * MIXMOM_TI + threadIdx.x, j = blockIdx.y * MIXMOM_TJ + threadIdx.y;
  if (i >= a.m || j >= a.m || i < j) return;
  const double v = fma(-a.s1[i], a.s1[j], a.acc[(long long)j * a.m + i]);
  a.out_cov[(long long)j * a.m + i] = v;
  a.out_cov[(long long)i * a.m + j] = v;
  if (i == j) {
    a.out_var[i] = v;
    a.out_mean[i] = a.s[i] + a.s1[i];
  }
}

}  // namespace agp
