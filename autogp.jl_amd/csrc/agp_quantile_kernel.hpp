// Quantiles of a Gaussian mixture, one independent search per (point, q): Statistics.quantile(::MixtureModel, q; tol, max_iter)
// of the reference (src/api.jl:559-596) applied to the per-point marginals Normal(mean_i, sqrt(var_i)) with weights w_i.
//
// The reference runs one vectorised loop over all points until every point has converged.  A converged point keeps its x and no
// point's update reads another's, so one search per point with its own early exit gives the same x bit for bit; a point that has
// not converged within max_iter checks reports it (the loop's `success` is the AND of these flags).  An update that leaves x
// bitwise unchanged leaves every later iteration identical (eps, x_max, x_min unchanged), so the search also stops there — with
// "not converged" and exactly the x that max_iter iterations would give — which bounds the kernel when tol is below what the
// fp64 CDF resolves, when tol <= 0, or when eps is NaN.  With tol <= 0, points where eps == 0 exactly can make the search go round
// a cycle of a few states instead; Brent's method finds its period lam, and the search then runs only the (max_iter - it) % lam
// updates that take it to the x of max_iter updates.
//
// The mixture CDF is Distributions' cdf(::UnivariateMixture): sum over components with w_i != 0 (exactly zero weights are
// skipped, so a NaN component at weight 0 contributes nothing) of w_i normcdf((x - mu_i) / sigma_i), with
//   normcdf(z) = erfc(-z * invsqrt2) / 2                              (StatsFuns' expression — written from memory)
//   sigma_i == 0: a step, 0 below mu_i, 1 above, 1/2 at x == mu_i     (the sigma = 0 convention — a choice, from memory)
// erfc is the device library's (its error against mpmath is pinned by tests/test_gpu_predict_quantile.py through
// agp_debug_math(which = 4)).  x depends on the CDF only through the branch decisions (signs of eps, |eps| < tol): two
// implementations that take the same decisions return the same x and iteration counts bit for bit.
//
// Layout: one wave per (point i, quantile k); the lanes stride over the components (lane l sums l, l + 64, ... in that order),
// a fixed xor butterfly combines the 64 partial sums (every lane ends with the same bits), and the update rule runs on scalar
// registers.  The summation order is a function of P alone, so a point's result depends only on its own components, q, tol,
// max_iter and the particle order — not on m, nq or the other points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace agp {

constexpr int MQ_WAVES = 4;                 // waves (searches) per 256-thread workgroup
constexpr double MQ_INVSQRT2 = 0.7071067811865476;      // IrrationalConstants.invsqrt2 as a Float64

// Julia's min / max on Float64: NaN if either argument is NaN; min(-0.0, 0.0) = -0.0, max(-0.0, 0.0) = 0.0.
__device__ __forceinline__ double jl_min(double a, double b) {
  if (a != a || b != b) return a + b;
  return (b < a || (__builtin_signbit(b) && !__builtin_signbit(a))) ? b : a;
}
__device__ __forceinline__ double jl_max(double a, double b) {
  if (a != a || b != b) return a + b;
  return (b > a || (__builtin_signbit(a) && !__builtin_signbit(b))) ? b : a;
}

__device__ __forceinline__ bool same_bits(double a, double b) {
  return __builtin_bit_cast(uint64_t, a) == __builtin_bit_cast(uint64_t, b);
}

// a value every lane holds with the same bits, moved to scalar registers (the loop's control flow is then provably uniform)
__device__ __forceinline__ double wave_uniform(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// normcdf((x - mu) / sigma) with the sigma == 0 step
__device__ __forceinline__ double mq_normcdf(double x, double mu, double sg) {
#pragma clang fp contract(off)
  if (sg == 0.0) return x < mu ? 0.0 : (x > mu ? 1.0 : 0.5);
  const double z = (x - mu) / sg;
  return 0.5 * erfc(-z * MQ_INVSQRT2);
}

// Transposes the components to one contiguous row per point and takes the square roots:
//   cm[i * Pp + j] = means[j * m + i], cs[i * Pp + j] = sqrt(vars[j * m + i])   for j < P; (0, 1) in the padding j in [P, Pp).
// sqrt is the correctly rounded one (llvm.sqrt.f64: v_sqrt_f64 with the scaling and the two Newton-Raphson correction steps).
__global__ __launch_bounds__(256) void k_mixture_pack(const double* __restrict__ means, const double* __restrict__ vars, int P, int Pp,
                                                      int m, double* __restrict__ cm, double* __restrict__ cs) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;        // (m * Pp < 2^31: checked by the host)
  if (g >= (unsigned)m * (unsigned)Pp) return;
  const unsigned i = g / (unsigned)Pp, j = g % (unsigned)Pp;
  double mu = 0.0, sg = 1.0;
  if (j < (unsigned)P) {
    const long long src = (long long)j * m + i;
    mu = means[src];
    sg = __builtin_sqrt(vars[src]);
  }
  cm[g] = mu;
  cs[g] = sg;
}

// One search: the quantile qk of the mixture whose packed row is (rm, rs) with weights cw (Pp entries each, Pp a multiple of 64, weight
// 0 in the padding), by all 64 lanes of one wave.  Every argument but `lane` is wave-uniform; x, conv and it come back with the same
// bits in every lane.  The one body of every search kernel (k_mixture_quantile here, k_series_mix_quantile in
// agp_series_quantile_kernel.hpp): a point's bits depend on its row, its weights, qk, tol and max_iter alone.
__device__ __forceinline__ void mq_search(const double* __restrict__ rm, const double* __restrict__ rs, const double* __restrict__ cw,
                                          int Pp, double qk, double tol, long long max_iter, int lane, double* out_x, int* out_conv,
                                          long long* out_it) {
#pragma clang fp contract(off)      // every product and sum rounded on its own, as the reference (and tests/_mixture_quantile_ref.py) do
  double x = 0.0, x_max = __builtin_inf(), x_min = -__builtin_inf();
  long long it = 0;
  int conv = 0;
  // Brent's cycle search on the state (x, x_max, x_min): saved at powers of two; period lam found at update `it` -> the x of
  // max_iter updates is the one (max_iter - it) % lam updates on, so the search runs to that limit instead
  double bx = 0.0, bX = x_max, bN = x_min;
  long long power = 1, lam = 0, limit = max_iter;
  bool cyc = false;
  while (it < limit) {
    double s = 0.0;
    for (int j = lane; j < Pp; j += 64) {
      const double w = cw[j];
      if (w != 0.0) s += w * mq_normcdf(x, rm[j], rs[j]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const double eps = wave_uniform(s) - qk;
    if (__builtin_fabs(eps) < tol) { conv = 1; break; }
    x_max = eps > 0.0 ? x : x_max;
    x_min = eps < 0.0 ? x : x_min;
    // 2^sign(x) * x + (x == 0) and 2^-sign(x) * x - (x == 0); sign(NaN) = NaN, sign(+-0) = +-0 (2^+-0 = 1)
    const double up = x > 0.0 ? 2.0 : (x < 0.0 ? 0.5 : (x == 0.0 ? 1.0 : x));
    const double dn = x > 0.0 ? 0.5 : (x < 0.0 ? 2.0 : (x == 0.0 ? 1.0 : x));
    const double z01 = x == 0.0 ? 1.0 : 0.0;
    const double x_hi = jl_min(x_max, up * x + z01);
    const double x_lo = jl_max(x_min, dn * x - z01);
    const double xn = eps < 0.0 ? (x + x_hi) / 2.0 : (x + x_lo) / 2.0;
    ++it;
    const bool fixed = same_bits(xn, x);
    x = xn;
    if (fixed) break;
    if (!cyc) {
      ++lam;
      if (same_bits(x, bx) && same_bits(x_max, bX) && same_bits(x_min, bN)) { cyc = true; limit = it + (max_iter - it) % lam; }
      else if (lam == power) { bx = x; bX = x_max; bN = x_min; power *= 2; lam = 0; }
    }
  }
  *out_x = x; *out_conv = conv; *out_it = it;
}

// out_x[k * m + i], out_conv / out_iters (may be null) likewise.  cw: Pp weights (0 in the padding).
__global__ __launch_bounds__(256) void k_mixture_quantile(const double* __restrict__ cm, const double* __restrict__ cs,
                                                          const double* __restrict__ cw, int Pp, int m, const double* __restrict__ q,
                                                          int nq, double tol, long long max_iter, double* __restrict__ out_x,
                                                          int32_t* __restrict__ out_conv, int32_t* __restrict__ out_iters) {
  const int lane = threadIdx.x & 63;
  const unsigned wid = blockIdx.x * MQ_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (m * nq < 2^31: the host)
  if (wid >= (unsigned)m * (unsigned)nq) return;
  const unsigned i = wid % (unsigned)m, k = wid / (unsigned)m;
  double x;
  long long it;
  int conv;
  mq_search(cm + (long long)i * Pp, cs + (long long)i * Pp, cw, Pp, q[k], tol, max_iter, lane, &x, &conv, &it);
  if (lane == 0) {
    const unsigned o = k * (unsigned)m + i;
    out_x[o] = x;
    if (out_conv) out_conv[o] = conv;
    if (out_iters) out_iters[o] = (int32_t)(it < 0x7fffffffLL ? it : 0x7fffffffLL);
  }
}

}  // namespace agp
