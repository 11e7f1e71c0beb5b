// The read-out of agp_predict_quantile_series_batch: forecast bands of many short series from the predictive launches' device outputs
// (k_series_predict's particle-major means and variances), without a trip through the host.  Three kernels on the call's stream:
//   k_series_mix_pack      per series: predict_mvn's raw-space transform with the series' own (slope, intercept), the correctly rounded
//                          sqrt, and the transpose into k_mixture_pack's row format — one contiguous row of Pp_s = ceil(P_s / 64) 64
//                          entries per (series, query), (0, 1) in the padding; the series' particles are gathered through its list.
//                          Its first workgroup per series also writes the particles' first_bad words (raw_components' rule) and the
//                          series' bad flag.
//   k_series_mix_quantile  one wave per (series, query, quantile): mq_search (agp_quantile_kernel.hpp) on that row — the body
//                          k_mixture_quantile runs, so a point's bits are those of agp_mixture_quantile on the series' stacked block.
//   k_series_mix_moments   one thread per (series, query): k_mixmom_marginal + k_mixmom_finish_marginal's arithmetic (space 0) — the
//                          sums about the raw mean of the first particle of positive weight, sequentially in the list's order, weight-0
//                          particles skipped, the same fma's — so the bits are agp_mixture_moments' on the stacked block.
// A series without particles, or with a bad flag, gets NaN (x, mean, var) and 0 (converged, iterations).  Every word a kernel reads
// was written earlier in the same call: by the uploads, the predictive launches or the pack kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "agp_args.hpp"
#include "agp_quantile_kernel.hpp"

namespace agp {

// largest s in [0, S) with off[s] * scale <= g, for g below off[S] * scale (series without queries are stepped over: off repeats)
__device__ __forceinline__ int series_of(const long long* __restrict__ off, int S, long long scale, long long g) {
  int lo = 0, hi = S;      // off[lo] * scale <= g < off[hi] * scale
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] * scale <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// grid (S, chunks): workgroup (s, c) packs elements c 256 + t, stepping by 256 chunks, of series s's m_s x Pp_s rows
__global__ __launch_bounds__(256) void k_series_mix_pack(SeriesQuantArgs a) {
  __shared__ int first[256];
  const int s = blockIdx.x, t = threadIdx.x;
  const long long pl0 = a.pl_off[s];
  const int Ps = (int)(a.pl_off[s + 1] - pl0);
  if (Ps == 0) return;                                   // (no mixture: nothing reads this series' flag or rows)
  const long long m = a.q_off[s + 1] - a.q_off[s];
  const int n = (int)(a.pt_off[s + 1] - a.pt_off[s]);
  const double sl = a.slope[s], ic = a.intercept[s], iv = a.ivar[s];
  const int32_t* __restrict__ pl = a.plist + pl0;
  if (blockIdx.y == 0) {
    // the info words, 256 particles at a time: the smallest failing query of each by an LDS atomic minimum
    const bool launched = n > 0 || m > 0;                // (the predictive wrote this series' info words)
    int any = 0;
    for (int c0 = 0; c0 < Ps; c0 += 256) {
      const int nc = Ps - c0 < 256 ? Ps - c0 : 256;
      first[t] = 0x7fffffff;
      __syncthreads();
      for (long long e = t; e < (long long)nc * m; e += 256) {      // (consecutive threads: consecutive queries of one particle)
        const int jj = (int)(e / m);
        const long long i = e - (long long)jj * m;
        const long long src = a.out_off[pl[c0 + jj]] + i;
        const double mr = (a.mean[src] - ic) / sl, vr = iv * a.var[src];
        if (!(__builtin_isfinite(mr) && vr >= 0.0)) atomicMin(&first[jj], (int)i);
      }
      __syncthreads();
      if (t < nc) {
        const int p = pl[c0 + t];
        const int word = first[t] == 0x7fffffff ? 0 : n + first[t] + 1;
        a.first_bad[p] = word;
        any |= (word != 0 || (launched && a.pred_info[p] != 0)) ? 1 : 0;
      }
      __syncthreads();
    }
    any = __syncthreads_or(any);
    if (t == 0) a.bad[s] = any != 0 ? 1 : 0;
  }
  const unsigned Pp = (unsigned)(a.w_off[s + 1] - a.w_off[s]);
  const unsigned nel = (unsigned)m * Pp;                 // (sum over the series < 2^31: checked by the host)
  double* __restrict__ cm = a.cm + a.row_off[s];
  double* __restrict__ cs = a.cs + a.row_off[s];
  for (unsigned g = blockIdx.y * 256u + t; g < nel; g += gridDim.y * 256u) {
    const unsigned i = g / Pp, j = g % Pp;
    double mu = 0.0, sg = 1.0;
    if (j < (unsigned)Ps) {
      const long long src = a.out_off[pl[j]] + i;
      mu = (a.mean[src] - ic) / sl;
      sg = __builtin_sqrt(iv * a.var[src]);
    }
    cm[g] = mu;
    cs[g] = sg;
  }
}

// wave wid of nq q_off[S]: out_x[wid] is series s's element (k, i), wid - nq q_off[s] = k m_s + i
__global__ __launch_bounds__(256) void k_series_mix_quantile(SeriesQuantArgs a) {
  const int lane = threadIdx.x & 63;
  const long long wid = (long long)blockIdx.x * MQ_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (< 2^31: the host)
  if (wid >= a.q_off[a.S] * a.nq) return;
  const int s = __builtin_amdgcn_readfirstlane(series_of(a.q_off, a.S, a.nq, wid));
  const long long q0 = a.q_off[s];
  const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)(a.q_off[s + 1] - q0));
  const unsigned local = (unsigned)__builtin_amdgcn_readfirstlane((int)(wid - q0 * a.nq));
  const unsigned i = local % m, k = local / m;
  const long long w0 = a.w_off[s];
  const int Pp = __builtin_amdgcn_readfirstlane((int)(a.w_off[s + 1] - w0));
  double x = __builtin_nan("");
  long long it = 0;
  int conv = 0;
  if (Pp != 0 && __builtin_amdgcn_readfirstlane(a.bad[s]) == 0) {
    const long long r0 = a.row_off[s] + (long long)i * Pp;
    mq_search(a.cm + r0, a.cs + r0, a.w + w0, Pp, a.q[k], a.tol, a.max_iter, lane, &x, &conv, &it);
  }
  if (lane == 0) {
    a.out_x[wid] = x;
    if (a.out_conv) a.out_conv[wid] = conv;
    if (a.out_iters) a.out_iters[wid] = (int32_t)(it < 0x7fffffffLL ? it : 0x7fffffffLL);
  }
}

// thread g of q_off[S]: series s's query i = g - q_off[s]
__global__ __launch_bounds__(256) void k_series_mix_moments(SeriesQuantArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.q_off[a.S]) return;
  const int s = series_of(a.q_off, a.S, 1, g);
  const long long i = g - a.q_off[s];
  const long long pl0 = a.pl_off[s];
  const int Ps = (int)(a.pl_off[s + 1] - pl0);
  double mean = __builtin_nan(""), var = __builtin_nan("");
  if (Ps != 0 && a.bad[s] == 0) {
    const int32_t* __restrict__ pl = a.plist + pl0;
    const double* __restrict__ w = a.w + a.w_off[s];
    const double sl = a.slope[s], ic = a.intercept[s], iv = a.ivar[s];
    int j0 = 0;
    while (j0 < Ps - 1 && !(w[j0] > 0.0)) ++j0;          // (the weights sum to 1: one of them is positive)
    // k_mixmom_marginal's statements (space 0) with the pivot at j0, then k_mixmom_finish_marginal's
    const double piv = (a.mean[a.out_off[pl[j0]] + i] - ic) / sl;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < Ps; ++j) {
      const double wj = w[j];
      if (wj == 0.0) continue;
      const long long src = a.out_off[pl[j]] + i;
      const double e = (a.mean[src] - ic) / sl, d = iv * a.var[src];
      const double r = e - piv;
      s1 = fma(wj, r, s1);
      s2 = fma(wj, fma(r, r, d), s2);
    }
    mean = piv + s1;
    var = fma(-s1, s1, s2);
  }
  if (a.out_mean) a.out_mean[g] = mean;
  if (a.out_var) a.out_var[g] = var;
}

// The mixture read-out of agp_predict_logpdf_series_batch, thread s of S: the log of series s's mixture density at its held-out
// vector, out[s] = M + log sum_{w_j > 0} w_j exp(lp_j - M), M = max_{w_j > 0} lp_j, over the series' list in ascending order (one
// thread, one order).  NaN when ANY particle of the series has info != 0, whatever its weight, and for a series without particles
// (the band's rule); exactly 0 for a series with particles and nothing held out (its particles were not launched: lp is not read).
__global__ __launch_bounds__(256) void k_series_mix_logp(SeriesMixLogpArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= a.S) return;
  const long long pl0 = a.pl_off[s];
  const int Ps = (int)(a.pl_off[s + 1] - pl0);
  double r = __builtin_nan("");
  if (Ps != 0) {
    if (a.q_off[s + 1] == a.q_off[s]) {
      r = 0.0;
    } else {
      const int32_t* __restrict__ pl = a.plist + pl0;
      const double* __restrict__ w = a.w + a.w_off[s];
      int bad = 0;
      double M = -__builtin_inf();
      for (int j = 0; j < Ps; ++j) {
        const int p = pl[j];
        bad |= a.info[p];
        if (w[j] > 0.0) M = fmax(M, a.lp[p]);
      }
      if (bad == 0) {
        double sum = 0.0;
        for (int j = 0; j < Ps; ++j)
          if (w[j] > 0.0) sum = fma(w[j], exp(a.lp[pl[j]] - M), sum);
        r = M + log(sum);
      }
    }
  }
  a.out[s] = r;
}

}  // namespace agp
