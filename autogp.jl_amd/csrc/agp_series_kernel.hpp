// Small-matrix value kernel: log N(xs_s; 0, K_p(ts_s) + noise_p I) of one particle on one SHORT series (n <= SERIES_MAX_N = 176 points)
// by ONE workgroup with everything in LDS — covariance, Cholesky factor, forward solve, log-det and the value itself; one launch
// scores many (series, particle) pairs (agp_logpdf_series_batch, agp_series.hip).  The reference's data sets have 135, 143 and 442
// points and its tutorials 6 to 18 particles: at those sizes the tiled sweeps (agp_chol_kernel.hpp: 128 x 128 tiles in HBM, launches per
// block column) are bound by launch latency and by padding behind a 128-pivot chain, and they serve one resident series at a time.
//
// k_series_logpdf<D> (256 threads, D = depth of the evaluation stack, 4 or 8), per workgroup:
//   1. ts, xs of the particle's series, its compiled program and parameters -> LDS;
//   2. per-point tables: sigma_cp of every ChangePoint node at ALL points of the series (n <= 176 <= 256: one 256-entry table per node
//      holds the whole series, so eval_program's sig[c * 256 + index] is indexed by the point's position itself);
//   3. the lower triangle of K + noise I by the general evaluator (eval_program<D, 4, 0>: the fm:: arithmetic of every other path)
//      straight into LDS as packed lower 16 x 16 column-major blocks — block (rb, cb) at blk_idx(rb, cb) * 256, the layout of
//      factor_diag_tile with nb = ceil(n / 16) block rows instead of 8; rows / columns past n are identity (cov_finalize);
//   4. right-looking 16 x 16-blocked Cholesky in LDS over the particle's own nb block steps: diagonal block + its inverse in one wave
//      (factor16), panel and trailing updates on v_mfma_f64_16x16x4 across the waves, the next diagonal block factored by wave 0
//      beside the trailing updates — lds_chol_steps of agp_lds_chol.hpp, the code factor_diag_tile runs on its eight block rows;
//   5. alpha = L^-1 xs carried along block by block (W r + one refinement step), sum log L_ii, alpha'alpha, first bad pivot ->
//      out_logpdf[p] = -(n log 2 pi + 2 sum log L_ii + alpha'alpha) / 2 (NaN on a bad pivot), out_info[p].
// No HBM workspace per particle, no finish kernel.
//
// k_series_logpdf<4, true> is the probe (agp_debug_series_factor): stages 1-3 are a load of the caller's matrix and right-hand side
// into the same LDS layout (series_lds(n, 0, 0, 0)), stages 4 and 5 are the statements below — the ones every production
// instantiation runs — and the packed blocks, alpha and the two partials of the value are written to HBM at the end.
//
// LDS budget (SeriesLds, agp_args.hpp): nb (nb + 1) / 2 blocks of 2 KiB — 90 KiB at n = 144 (45 blocks), 132 KiB at n = 176 (66) —
// + Wl 2 KiB (inverse of the current diagonal block) + ts, rvec, avec 3 x 8 np B (4.1 KiB at 176) + exponential table 1 KiB
// + parameters and opcodes (a few hundred bytes for the trees the prior draws, 6.6 KiB for a 255-node tree) + 2 KiB per ChangePoint node.
// One workgroup may declare 160 KiB: at n = 176 that leaves 160 - 132 - 7.1 = 20.9 KiB, i.e. 10 per-point tables beside a small program
// (the host refuses a particle whose total exceeds 160 KiB).  Short series need little (n <= 64: 10 blocks, ~28 KiB), so the host
// launches one grid per LDS class and several workgroups share a CU there.
//
// A particle's bits depend on its own series, program, parameters and noise only: the LDS map is a function of the particle's own
// sizes, no value crosses workgroups, and every reduction runs in a fixed order.
//
// k_series_logpdf_grad<D, GS> (agp_logpdf_grad_series_batch) is the value kernel with the gradient behind it, in the same workgroup and
// the same LDS: stages 1-5 are the statements of k_series_logpdf (one body, series_body; the value's bits are the value kernel's), then
//   G1. the diagonal blocks L(i,i)^-T by forward substitution, in place;
//   G2. Z = L^-T in place, block column by block column: Z(j,i) = -[sum_{j<=k<i} Z(j,k) L(i,k)'] L(i,i)^-T sits where L(i,j) sat (a
//       second copy of the blocks does not fit at n = 176), so a column's results wait in registers until every wave has read
//       row i of L; products on v_mfma_f64_16x16x4 with the operand reads of the panel step;
//   G3. alpha = Z beta into its own vector;
//   G4. per lower block (rb, cb), one wave: K^-1(rb,cb) = sum_{k>=rb} Z(rb,k) Z(cb,k)' by an MFMA chain into registers — never stored —
//       G = 1/2 (alpha alpha' - K^-1) on the spot, and grad_elements (the tiled sweep's reverse-mode pass, private tape of GS nodes) on
//       the lane's four elements; DIAGONAL BLOCKS ARE EVALUATED IN FULL AT WEIGHT 1, off-diagonal blocks at weight 2, rows / columns
//       past n at weight 0 (Z's padding is identity and must not leak); tr G from the diagonal elements;
//   G5. thread -> wave -> the four waves in order -> out_grad through gmap (the caller's parameter order), out_gnoise.
// On a bad pivot G1-G4 are skipped and NaN is written.  The LDS map is series_grad_lds (agp_args.hpp): alpha, the gradient program and
// the reduction scratch in front of the blocks, and a second per-point table per ChangePoint node (1 - sigma, see grad_elements' CSIG);
// at n = 176 a chain of 4 ChangePoint nodes (9 nodes, 13 parameters, 8 tables) fits, 5 do not.
// An LDS tape (LdsTape: 8 nodes x 4 x 256 doubles = 64 KiB) would fit only beside short series' blocks; it is not built — see
// profiles/series_grad_perf.txt.
//
// k_series_predict<D> (agp_predict_series_batch) is the value kernel with the posterior at the series' own query times behind it, in the
// same workgroup and the value kernel's own LDS map (series_pred_lds): stages 1-5 as above, then
//   P1. the diagonal blocks L(i,i)^-T in place (G1's statements: series_diag_inv_t);
//   P2. per block of 16 query times, one wave, no workgroup barrier: K21 by the evaluator, VT = K21 L^-T block row by block row on
//       v_mfma_f64_16x16x4 with the finished blocks in registers, mean = VT beta, var = k(t*,t*) - rowsums(VT^2) + noise_pred
//       (series_predict_blocks).  sigma_cp at the query times sits in the per-point tables' entries 192 .. 255.
// The gradient kernel's full Z = L^-T is not formed (n^3 / 3 flops and nb - 1 barrier pairs for n^2 m of work).  An empty series with
// query points gives the prior predictive (series_prior_predict).  On a bad pivot NaN is written to the particle's whole block.
//
// k_series_predict_logpdf<D> (agp_predict_logpdf_series_batch) is the value kernel on the JOINT points of a series — its n training
// points followed, without padding, by its m query points, N = n + m <= SERIES_MAX_N — read out over the query rows alone: the
// log-density of the held-out values y under the particle's posterior predictive (predict_proba), by the route of
// agp_predict_logpdf_batch: with L the factor of [K11 + noise I, K12; K21, K22 + noise_pred I] and z = L^-1 [xs; y],
//   log p(y | xs) = -(m log 2 pi + 2 sum_{k >= n} log L_kk + sum_{k >= n} z_k^2) / 2.
// One body (series_body, selected by the argument type SeriesProbaArgs), the value kernel's LDS map at N points; it differs in
//   1. the loads: tpt = [ts | ts_pred], rvec = [xs | y_pred] (the train / query split falls anywhere inside a 16-block);
//   3. the diagonal: noise[p] for index < n, noise_pred[p] for index in [n, N); rows / columns past N identity as ever;
//   the read-out: both reductions (fixed order, as above) over the rows [n, N) alone, + m log|y_slope[s]| (the density of the raw
//      values), and optionally the per-point terms -(log 2 pi + z_k^2) / 2 - log L_kk + log|y_slope[s]| of those rows — the density of
//      held-out point k - n given the training data and the held-out points before it — particle-major behind out_off.
// Stages 2, 4 and 5 are the value kernel's statements over N points.  out_info[p] = the first bad pivot of the joint factor (1 .. n:
// K11; n + k: leading minor k of the predictive covariance), NaN then in out_lp[p] and the particle's whole terms block.  n = 0 (the
// prior predictive) takes the same code; m = 0 is never launched (the host answers 0).
//
// k_series_predict_sample<D> (agp_predict_sample_series_batch) is the held-out twin with the query rows' right-hand side 0 (the
// branches of the joint points are shared: the trait JOINT of series_body) and another read-out: after stage 5 the query rows of the
// packed blocks are [L21 L22] with L22 = chol(Sigma*) and avec[0, n) = L11^-1 xs, so the component mean mu* = L21 a, the component
// covariance Sigma* = L22 L22' and the samples mu* + L22 z of predict_mvn / rand are read out of rows [n, N) in the same workgroup and
// the value kernel's LDS map (series_sample_readout); k_series_sample_fill behind the launches turns the block of a series with a
// failed particle into NaN.
//
// k_series_predict_sum<D> (agp_predict_sum_series_batch) is the predictive kernel on a sum of GPs, X = F_1 + .. + F_M + noise: the
// posterior of every latent part and of the observable at the series' query times (GP.infer_gp_sum, predict_sum), by the coded-points
// route of agp_infer_gp_sum_batch.  The particle's program is the composite K_1 SEL_1 * K_2 SEL_2 * + .. (append_composite); a
// selector leaf reads a per-point table like a ChangePoint node's (eval_program's OP_SEL; ProgHdr::n_cp counts both kinds, tables
// numbered in program order), so the LDS map is series_pred_lds as it stands.  One body again (argument type SeriesSumArgs; the
// predictive branches P1, P2 and the map are shared with k_series_predict through the trait PRED).  It differs in
//   2. the tables: SEL_i holds 1.0 at every training point — they are the observable, code 0 — so K11 is the sum of the parts;
//   P2. the rows: series s with m query times has (M + 1) m joint rows g in the reference's order F_1(T*) .. F_M(T*), X(T*); row g is
//       component i = g / m at time tq[g % m] with code i < M ? i + 1 : 0, and SEL_j's entry at the row's query slot is
//       (code == 0 || code == j).  16 consecutive rows belong to one wave as 16 queries do, whatever their codes: every lane has its own
//       slot entry.  var = (k** - sum VT^2) + [1e-8 + (i == M ? noise_pred : 0)]: JITTER on every row, noise_pred on the observable's
//       only.  Code and addend of a row are recomputed from g where they are used, not carried through the block loop;
//   the read-out, in the lanes that hold the row (k_sum_readout's statements, no further launch): raw mean (mean - b) / a, + b / a on
//       the F_1 rows, raw variance (1 / (a a)) var, quantiles fma(sqrt(var), z_k, mean); a row whose raw variance is negative or NaN or
//       whose raw mean is not finite marks the particle with min(g + 1) in an LDS word (ds_min), and behind ONE workgroup barrier a
//       marked particle's whole blocks become NaN and out_info[p] = n + g + 1 (series_sum_rows).
// An empty series with query points gives the prior of every part through the same rows (series_prior_predict_sum).  On a bad pivot
// NaN is written to all of the particle's outputs.  244 / 232 VGPRs (D = 4 / 8), no scratch.  The X rows are not formed as the sum of
// the F rows' VT: a second set of eleven register blocks does not fit beside the first.
#pragma once
#include <type_traits>
#include "agp_common.hpp"
#include "agp_args.hpp"
#include "agp_cov_kernel.hpp"
#include "agp_lds_chol.hpp"         // mfma, blk_idx, lds_chol_steps
#include "agp_grad_elements.hpp"    // grad_elements, RegTape, ScratchAcc
#include "agp_ndtri.hpp"
#include "agp_philox.hpp"

namespace agp {

// block b of the packed lower block triangle, counted row by row -> its block row rb and block column cb
__device__ __forceinline__ void series_blk_rc(int b, int& rb, int& cb) {
  rb = 0;
  while ((rb + 1) * (rb + 2) / 2 <= b) ++rb;
  cb = b - rb * (rb + 1) / 2;
}

// sigma_cp (src/GP.jl:481-483) of every ChangePoint node at time t -> entry `slot` of the node's per-point table (cov_prologue's arithmetic)
// SEL (composite programs of the decomposition twin): also the selector leaves' entries for a point of component code `code` —
// 1 where the point is the observable (code 0) or the leaf's own component — tables numbered in program order across both kinds.
template <bool SEL = false>
__device__ __forceinline__ void series_sigma_cp(const ProgHdr& h, const int* ops, const double* prm, double* sig, int slot, double t,
                                                [[maybe_unused]] int code = 0) {
  int q = 0, c = 0;
  for (int ip = 0; ip < h.n_ops; ++ip) {
    const int o = ops[ip];
    if (o == OP_CP || o == OP_CP_SWAP) {
      const double loc = prm[q], sc = prm[q + 1];
      sig[c * 256 + slot] = 0.5 * (1.0 + tanh((loc - t) / sc));
      ++c;
    }
    if constexpr (SEL) {
      if (o == OP_SEL) {
        sig[c * 256 + slot] = (code == 0 || code == (int)prm[q]) ? 1.0 : 0.0;
        ++c;
      }
    }
    q += prm_count(o);
  }
}

// What the decomposition twin's rows need beside the predictive twin's arguments (series_predict_blocks<D, true>): the series'
// query count m and transform, the quantiles, and the LDS word that collects the first row without a raw marginal.
struct SeriesSumRows {
  int m, M, nq;              // query times of the series, components, quantiles per row
  double slope, icpt;        // scaled = slope raw + icpt
  const double* z;           // [nq]
  double* ox;                // the particle's (rows, nq) block of out_x
  int* rowbad;               // LDS: min over the failed rows of g + 1 (INT_MAX: none)
};

// G1 / P1: every diagonal block L(i,i) -> L(i,i)^-T in place (the whole block, zeros below the diagonal), one block per wave and
// pass, column c of L(i,i)^-1 by forward substitution in lane c (the reads of L are broadcasts).  No barrier inside.
__device__ __forceinline__ void series_diag_inv_t(double* sm, int nb, int w, int l) {
  for (int i = w; i < nb; i += 4) {
    double* blk = sm + blk_idx(i, i) * 256;
    if (l < 16) {
      double wv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double s = (r == l) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < r; ++k) s = fma(-blk[k * 16 + r], wv[k], s);
        wv[r] = s / blk[17 * r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) blk[r * 16 + l] = wv[r];      // Z(i,i)[c][r] = W[r][c]: the whole block, zeros below the diagonal
    }
  }
}

// P2: the posterior at the mq query times tq of one particle, from the factor as P1 leaves it (off-diagonal blocks L(i,k), diagonal
// slots L(i,i)^-T, beta = L^-1 x in avec; nb = 0: the prior).  Query block qb (16 times) belongs to wave qb % 4, which runs its
// blocks without a workgroup barrier:
//   sigma_cp of its 16 times -> entries SERIES_QSLOT + 16 w .. of every per-point table (wave-local; stage 2's arithmetic);
//   for jb = 0 .. nb - 1:  K21(jb) by the evaluator on stage 3's lane map (lane (i = l%16, q = l/16) <-> query i, training points
//     16 jb + q + 4 e; columns past n: 0), VT(jb) = (K21(jb) - sum_{k<jb} VT(k) L(jb,k)') L(jb,jb)^-T on v_mfma_f64_16x16x4 — a result
//     register r IS the operand slice s4 = r, so the finished blocks stay in registers (VT[k], statically indexed: the k-loop is
//     unrolled over the cap's 11 blocks behind wave-uniform guards) — and the lane's share of mean_i = sum_j VT[i][j] beta_j and of
//     sum_j VT[i][j]^2, ascending in (jb, e);
//   "block" nb: k(t*_i, t*_i) through the same call of the evaluator, row and column both the query;
//   the four lane groups of a row in the order ((q0 + q1) + q2) + q3 -> out_mean, out_var = (k** - sum VT^2) + noise_pred.
// Rows past mq evaluate the last query again and are not written; beta's padding is 0 and VT's columns past n are exactly 0
// (K21 masked, L's padding identity).
template <int D, bool SUM = false>
__device__ __forceinline__ void series_predict_blocks(const ProgHdr& h, const int* ops, const double* prm, double* sig, const double* tpt,
                                                      const double* avec, const double* etab, const double* sm, int n, int nb,
                                                      const double* tq, int mq, double noise_pred, double* om, double* ov,
                                                      [[maybe_unused]] const SeriesSumRows* sr = nullptr) {
  constexpr int E = 4, EV = D > 4 ? 2 : 4, NBMAX = SERIES_MAX_N / 16;
  static_assert(NBMAX * 16 == SERIES_MAX_N, "the cap is whole blocks");
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, l15 = l & 15, lq = l >> 4;
  const int slot = SERIES_QSLOT + 16 * w + l15;
  for (int qb = w; qb * 16 < mq; qb += 4) {
    const int qi = qb * 16 + l15;
    int tix = qi < mq ? qi : mq - 1;
    [[maybe_unused]] int code = 0;
    if constexpr (SUM) {      // row g of the (M + 1) m coded rows: component i = g / m (code i + 1; the observable, last, 0) at query time g % m
      const int i = tix / sr->m;
      tix -= i * sr->m;
      code = i < sr->M ? i + 1 : 0;
    }
    const double t = tq[tix];
    if (SUM || h.n_cp > 0) {
      if (l < 16) series_sigma_cp<SUM>(h, ops, prm, sig, slot, t, code);
      __builtin_amdgcn_wave_barrier();      // (LDS operations of one wave complete in order: its own lanes' entries, no workgroup barrier)
    }
    d4 VT[NBMAX];
#pragma unroll
    for (int k = 0; k < NBMAX; ++k) VT[k] = d4{0.0, 0.0, 0.0, 0.0};
    double ms = 0.0, ss = 0.0, kd = 0.0;
    for (int jb = 0; jb <= nb; ++jb) {
      const bool self = jb == nb;
      double out[E];
      int ci[E];
#pragma unroll
      for (int e = 0; e < E; ++e) ci[e] = self ? slot : jb * 16 + lq + 4 * e;
      // (the deep stack takes its four elements two at a time: its registers and the finished blocks' share one budget)
#pragma unroll
      for (int e0 = 0; e0 < E; e0 += EV) {
        double tr[EV], tc[EV], lt[EV], o2[EV];
        int ri[EV], c2[EV];
#pragma unroll
        for (int e = 0; e < EV; ++e) {
          tr[e] = t;
          ri[e] = slot;
          tc[e] = self ? t : tpt[ci[e0 + e]];
          c2[e] = ci[e0 + e];
          lt[e] = 0.0;
        }
        eval_program<D, EV, 0>(h, ops, prm, sig, tr, tc, ri, c2, lt, o2, etab);
#pragma unroll
        for (int e = 0; e < EV; ++e) out[e0 + e] = o2[e];
      }
      if (self) { kd = out[0]; break; }
      d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < NBMAX - 1; ++k)
        if (k < jb) {
          const double* lb = sm + blk_idx(jb, k) * 256;
          double fa[4];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) fa[s4] = lb[64 * s4 + l];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) acc = mfma(fa[s4], VT[k][s4], acc);      // += VT(k) L(jb,k)'
        }
      const double* zb = sm + blk_idx(jb, jb) * 256;
      double fw[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) fw[s4] = zb[l15 * 16 + 4 * s4 + lq];      // L(jb,jb)^-1 (l15, 4 s4 + lq), as in G2
      d4 res = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) res = mfma(fw[s4], (ci[s4] < n ? out[s4] : 0.0) - acc[s4], res);
#pragma unroll
      for (int k = 0; k < NBMAX; ++k)
        if (k == jb) VT[k] = res;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ms = fma(res[e], avec[ci[e]], ms);
        ss = fma(res[e], res[e], ss);
      }
    }
    const double mean = ((__shfl(ms, l15) + __shfl(ms, l15 + 16)) + __shfl(ms, l15 + 32)) + __shfl(ms, l15 + 48);
    const double sq = ((__shfl(ss, l15) + __shfl(ss, l15 + 16)) + __shfl(ss, l15 + 32)) + __shfl(ss, l15 + 48);
    if constexpr (SUM) {
      // the read-out in the same lanes (k_sum_readout's statements); code and addend of the row recomputed from g
      if (l < 16 && qi < mq) {
        const int i = qi / sr->m;
        const double var = (kd - sq) + (1e-8 + (i == sr->M ? noise_pred : 0.0));      // JITTER on every row, noise_pred on X(T*)
        double mr = (mean - sr->icpt) / sr->slope;
        if (i == 0) mr = mr + sr->icpt / sr->slope;      // (the intercept counted once: on the F_1 rows)
        const double vr = (1.0 / (sr->slope * sr->slope)) * var;
        const bool ok = isfinite(mr) && vr >= 0.0;
        if (!ok) atomicMin(sr->rowbad, qi + 1);
        const double sd = ok ? sqrt(vr) : __builtin_nan("");
        om[qi] = mr;
        ov[qi] = vr;
        double* xo = sr->ox + (long long)qi * sr->nq;
        for (int k = 0; k < sr->nq; ++k) xo[k] = fma(sd, sr->z[k], mr);
      }
    } else if (l < 16 && qi < mq) {
      om[qi] = mean;
      ov[qi] = (kd - sq) + noise_pred;
    }
  }
}

// The prior predictive of a particle on an EMPTY series (n = 0, mq > 0 query times): mean 0, var = k(t*, t*) + noise_pred — the
// read-out above with no block.  Stages its own program (stage 1's statements without the points).
template <int D>
__device__ __forceinline__ void series_prior_predict(const SeriesPredArgs& a, int p, double* smem) {
  const int tid = threadIdx.x;
  const ProgHdr h = a.hdr[p];
  const SeriesLds m = series_pred_lds(0, h.n_ops, h.n_prm, h.n_cp);
  double* etab = smem + m.o_etab;
  double* prm = smem + m.o_prm;
  int* ops = reinterpret_cast<int*>(smem + m.o_ops);
  double* sig = smem + m.o_sig;
  if (AGP_EXP_TABLE && tid < AGP_EXP_TAB_N) etab[tid] = fm::c_exp_tab[tid];
  for (int i = tid; i < h.n_prm + 2; i += 256) prm[i] = a.prm[h.prm_off + i];
  for (int i = tid; i < h.n_ops; i += 256) ops[i] = (int)a.ops[h.op_off + i];
  __syncthreads();
  const long long q0 = a.q_off[a.series[p]];
  const int mq = (int)(a.q_off[a.series[p] + 1] - q0);
  series_predict_blocks<D>(h, ops, prm, sig, smem, smem, etab, smem + m.o_blk, 0, 0, a.ts_pred + q0, mq, a.noise_pred[p],
                           a.out_mean + a.out_off[p], a.out_var + a.out_off[p]);
}

// The decomposition twin's rows of one particle (P2 on the (M + 1) mq coded rows, read out in the same lanes) and, behind ONE
// workgroup barrier, the row-level verdict: a particle with a row whose raw variance is negative or NaN, or whose raw mean is not
// finite, has NaN in its whole blocks.  Returns 0, or the smallest such g + 1 (the same in every thread).  rowbad: an LDS word no
// wave still reads (Wl's first: the value's reduction has been read by the wave that sets it).
template <int D>
__device__ __forceinline__ int series_sum_rows(const SeriesSumArgs& a, int p, const ProgHdr& h, const int* ops, const double* prm, double* sig,
                                               const double* tpt, const double* avec, const double* etab, const double* sm, int n, int nb,
                                               long long q0, int mq, int* rowbad) {
  const int tid = threadIdx.x;
  const int sidx = a.series[p];
  const int rows = (a.M + 1) * mq;
  double* om = a.out_mean + a.out_off[p];
  double* ov = a.out_var + a.out_off[p];
  double* ox = a.out_x + (long long)a.nq * a.out_off[p];
  const SeriesSumRows sr{mq, a.M, a.nq, a.y_slope[sidx], a.y_intercept[sidx], a.z, ox, rowbad};
  series_predict_blocks<D, true>(h, ops, prm, sig, tpt, avec, etab, sm, n, nb, a.ts_pred + q0, rows, a.noise_pred[p], om, ov, &sr);
  __syncthreads();
  const int rb = *rowbad;
  if (rb == 0x7fffffff) return 0;
  for (int g = tid; g < rows; g += 256) { om[g] = __builtin_nan(""); ov[g] = __builtin_nan(""); }
  for (long long i = tid; i < (long long)rows * a.nq; i += 256) ox[i] = __builtin_nan("");
  return rb;
}

// ... on an EMPTY series: the prior of every part — means 0, var_i = K_i(t, t) + 1e-8, X also + noise_pred — through the same rows
// (series_prior_predict's staging).  Returns series_sum_rows' verdict.
template <int D>
__device__ __forceinline__ int series_prior_predict_sum(const SeriesSumArgs& a, int p, double* smem) {
  const int tid = threadIdx.x;
  const ProgHdr h = a.hdr[p];
  const SeriesLds m = series_pred_lds(0, h.n_ops, h.n_prm, h.n_cp);
  double* etab = smem + m.o_etab;
  double* prm = smem + m.o_prm;
  int* ops = reinterpret_cast<int*>(smem + m.o_ops);
  double* sig = smem + m.o_sig;
  int* rowbad = reinterpret_cast<int*>(smem);
  if (AGP_EXP_TABLE && tid < AGP_EXP_TAB_N) etab[tid] = fm::c_exp_tab[tid];
  for (int i = tid; i < h.n_prm + 2; i += 256) prm[i] = a.prm[h.prm_off + i];
  for (int i = tid; i < h.n_ops; i += 256) ops[i] = (int)a.ops[h.op_off + i];
  if (tid == 0) *rowbad = 0x7fffffff;
  __syncthreads();
  const long long q0 = a.q_off[a.series[p]];
  const int mq = (int)(a.q_off[a.series[p] + 1] - q0);
  return series_sum_rows<D>(a, p, h, ops, prm, sig, smem, smem, etab, smem + m.o_blk, 0, 0, q0, mq, rowbad);
}

// The read-out of the sampling twin: from the joint factor as stage 5 leaves it (rows [ntr, ntr + m) of the packed blocks are
// [L21 L22], L22 = chol(Sigma*); a = L11^-1 xs in avec[0, ntr)), in this order:
//   S1. mu*_i = sum_{k < ntr} L(ntr + i, k) a_k, one thread per query row, k ascending -> mu (LDS) and out_mean = (mu* - b) / slope;
//   S2. the samples of this particle (its CSR list smp), 16 per wave and pass, groups round-robin over the waves, no workgroup barrier:
//       x(i, j) = mu*_i + sum_k L22(i, k) sgn z_k(j) on v_mfma_f64_16x16x4 — the accumulator starts at mu*_i (the training columns
//       contribute the same to every sample: S1's sum is not repeated per sample) and runs over the query columns in 16-blocks of the
//       QUERY index, whatever ntr % 16 is.  Lane (j = l % 16, q = l / 16) feeds z of query points 16 kb + 4 q + s4 at step s4 — the
//       four words of ONE Philox block (4 kb + q, j, 1, 0), none wasted — so the L operand runs over k in the same order:
//       lane (i = l % 16, q) reads L22(16 rb + i, 16 kb + 4 q + s4).  Every element is one chain in a fixed order over k that involves
//       no other sample: its bits do not depend on R or on which samples share a group.  The accumulators of up to six row blocks live
//       in registers (statically indexed behind wave-uniform guards, as VT in series_predict_blocks), so z is formed once per block
//       column for m <= 96 and twice above;
//   S3. out_cov: per lower 16 x 16 block (rb, cb) of the query range, one wave, Sigma*(rb, cb) = sum_{k <= cb} L22(rb, k) L22(cb, k)'
//       by an MFMA chain; elements on and below the diagonal are stored at (r, c) AND at (c, r): both triangles, exactly symmetric.
// L22 is read through ONE accessor on the joint blocks (row / column ntr + i, masked with a select above the diagonal and past m: what
// sits there — zeros, identity padding or poison — never reaches an operand); no query-aligned copy is staged (it would not fit beside
// the blocks at the cap).  On a bad pivot the particle's mean and covariance blocks are NaN and no sample is drawn.
__device__ __forceinline__ void series_sample_readout(const SeriesSampleArgs& a, int p, const double* sm, const double* avec, double* mu,
                                                      bool isbad, int ntr, int m) {
  constexpr int RBP = 6;      // row blocks per pass of S2 (the cap has 11)
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, l15 = l & 15, lq = l >> 4;
  const int sidx = a.series[p];
  const long long q0 = a.q_off[sidx];
  const double slope = a.y_slope[sidx], icpt = a.y_intercept[sidx];
  const double nanv = __builtin_nan("");
  // ---- S1 ----
  if (tid < m) {
    const int row = ntr + tid, rb = row >> 4, r = row & 15;
    double s = 0.0;
    for (int k = 0; k < ntr; ++k) s = fma(sm[blk_idx(rb, k >> 4) * 256 + (k & 15) * 16 + r], avec[k], s);
    mu[tid] = s;
    if (a.out_mean != nullptr) a.out_mean[a.out_off[p] + tid] = isbad ? nanv : (s - icpt) / slope;
  }
  if (isbad) {
    if (a.out_cov != nullptr)
      for (int i = tid; i < m * m; i += 256) a.out_cov[a.cov_off[p] + i] = nanv;
    return;
  }
  __syncthreads();
  auto Lq = [&](int ir, int ic) -> double {      // L22(ir, ic); exactly 0 above the diagonal and for rows past m
    const bool on = ic <= ir && ir < m;
    const int jr = ntr + (on ? ir : 0), jc = ntr + (on ? ic : 0);
    const double v = sm[blk_idx(jr >> 4, jc >> 4) * 256 + (jc & 15) * 16 + (jr & 15)];
    return on ? v : 0.0;
  };
  const int nqb = (m + 15) >> 4;
  // ---- S2 ----
  {
    const long long s0 = a.smp_off[p];
    const int cnt = (int)(a.smp_off[p + 1] - s0);
    const double sgn = slope > 0.0 ? 1.0 : -1.0;
    const unsigned long long seed = a.seeds[sidx];
    double* ox = a.out_x + a.R * q0;
    for (int g = w; g * 16 < cnt; g += 4) {
      const int js = g * 16 + l15;
      const bool live = js < cnt;
      const long long j = live ? (long long)a.smp[s0 + js] : 0;
      // (row blocks in passes of RBP: the accumulators of one pass and the Philox state share the register budget; a series with
      // more than RBP query blocks forms z a second time for the later rows — every element's chain over k stays what it was)
      for (int rb0 = 0; rb0 < nqb; rb0 += RBP) {
        d4 acc[RBP];
#pragma unroll
        for (int u = 0; u < RBP; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = (rb0 + u) * 16 + 4 * r + lq;
            acc[u][r] = i < m ? mu[i] : 0.0;
          }
        const int kend = rb0 + RBP < nqb ? rb0 + RBP : nqb;
        for (int kb = 0; kb < kend; ++kb) {
          double zz[4];
          if (a.zin != nullptr) {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              const int i = kb * 16 + 4 * lq + s4;
              zz[s4] = (live && i < m) ? sgn * a.zin[a.R * q0 + j * m + i] : 0.0;
            }
          } else {
            const Philox4 b = philox4x64_10((uint64_t)(kb * 4 + lq), (uint64_t)j, 1, 0, seed, 0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              const int i = kb * 16 + 4 * lq + s4;
              zz[s4] = (live && i < m) ? sgn * ndtri(philox_uniform(b.w[s4])) : 0.0;
            }
          }
#pragma unroll
          for (int u = 0; u < RBP; ++u)
            if (rb0 + u >= kb && rb0 + u < nqb) {
#pragma unroll
              for (int s4 = 0; s4 < 4; ++s4) acc[u] = mfma(Lq((rb0 + u) * 16 + l15, kb * 16 + 4 * lq + s4), zz[s4], acc[u]);
            }
        }
        // accumulator (lane, reg r) of row block rb: query row 16 rb + 4 r + l / 16 of sample l % 16
#pragma unroll
        for (int u = 0; u < RBP; ++u)
          if (rb0 + u < nqb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = (rb0 + u) * 16 + 4 * r + lq;
              if (live && i < m) ox[j * m + i] = (acc[u][r] - icpt) / slope;
            }
          }
      }
    }
  }
  // ---- S3 ----
  if (a.out_cov != nullptr) {
    double* oc = a.out_cov + a.cov_off[p];
    const double s2 = slope * slope;
    const int nblk = nqb * (nqb + 1) / 2;
    for (int b = w; b < nblk; b += 4) {
      int rb, cb;
      series_blk_rc(b, rb, cb);
      d4 x = d4{0.0, 0.0, 0.0, 0.0};
      for (int kb = 0; kb <= cb; ++kb) {
        double fa[4], fb[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const int k = kb * 16 + 4 * s4 + lq;
          fa[s4] = Lq(cb * 16 + l15, k);
          fb[s4] = Lq(rb * 16 + l15, k);
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) x = mfma(fa[s4], fb[s4], x);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rb * 16 + l15, col = cb * 16 + 4 * r + lq;
        if (row < m && col <= row) {
          const double v = x[r] / s2;
          oc[col * m + row] = v;
          oc[row * m + col] = v;
        }
      }
    }
  }
}

// ---- the HMC twin's chain (k_series_hmc): state in LDS (series_hmc_lds), control in registers — the same in every thread ----
enum { HMC_ST_NOISE, HMC_ST_ZN, HMC_ST_ZSN, HMC_ST_MN, HMC_ST_GN, HMC_ST_GZN, HMC_ST_LP, HMC_ST_BAD };      // entries of st
enum { HMC_PH_INIT, HMC_PH_START, HMC_PH_LEAP, HMC_PH_FINAL };      // what the evaluation that has just finished was for
enum { HMC_EV_GRAD, HMC_EV_GNOISE, HMC_EV_VALUE };                  // what an evaluation must deliver
struct HmcLds {
  double *th, *z, *zs, *mom, *grd, *tf, *st;
  int *cls, *smap;
};
struct HmcCtl {
  int ph = HMC_PH_INIT, mode = HMC_EV_VALUE;
  int it = 0, mv = 0, step = 0, L = 0, nsel = 0;
  int nrej = 0, pacc = 0, pmade = 0, stop = 0, moved = 0;
  int cnt[4] = {0, 0, 0, 0};
  double eps = 0.0, U0 = 0.0, K0 = 0.0, logu = 0.0;
};
// (the control state lives in LDS between two calls of series_hmc_ctl — st[HMC_ST_CTL ..] — not in registers across an evaluation)
constexpr int HMC_ST_CTL = 8;
static_assert(sizeof(HmcCtl) <= sizeof(double) * (HMC_ST_N - HMC_ST_CTL), "the control state fits the chain's scalars");
__device__ __forceinline__ HmcCtl* hmc_ctl_ptr(double* smem, const SeriesHmcLds& m) { return reinterpret_cast<HmcCtl*>(smem + m.o_st + HMC_ST_CTL); }
__device__ __forceinline__ HmcLds hmc_lds_ptrs(double* smem, const SeriesHmcLds& m) {
  HmcLds hp;
  hp.th = smem + m.o_th; hp.z = smem + m.o_z; hp.zs = smem + m.o_zs; hp.mom = smem + m.o_mom; hp.grd = smem + m.o_grd;
  hp.cls = reinterpret_cast<int*>(smem + m.o_cls); hp.smap = hp.cls + (m.o_tf - m.o_cls);
  hp.tf = smem + m.o_tf; hp.st = smem + m.o_st;
  return hp;
}
// theta = transform(z) of class c (src/Model.jl:24-49) and d theta / d z at theta
__device__ __forceinline__ double hmc_transform(const double* tf, int c, double z) {
  const double mu = tf[3 * c], sg = tf[3 * c + 1], sc = tf[3 * c + 2];
  const double x = fma(sg, z, mu);
  return sc == 0.0 ? exp(x) : sc / (1.0 + exp(-x));
}
__device__ __forceinline__ double hmc_dtheta(const double* tf, int c, double th) {
  const double sg = tf[3 * c + 1], sc = tf[3 * c + 2];
  return sc == 0.0 ? sg * th : sg * th * (1.0 - th / sc);
}

// Stage 1 of the HMC twin, behind the value kernel's: the particle's latent state, classes and slot map, the class table and the
// gradient program's tables (k_grad_contract's staging without the parameter values) -> LDS; its block of the trace -> NaN.
__device__ __forceinline__ void series_hmc_stage(const SeriesHmcArgs& a, int p, const SeriesHmcLds& m, double* smem) {
  const int tid = threadIdx.x;
  const SeriesHmcParams& q = *a.hm;
  const GProgHdr g = a.ghdr[p];
  const HmcLds hp = hmc_lds_ptrs(smem, m);
  double* gprm = smem + m.o_gprm;
  int32_t* gpoff = reinterpret_cast<int32_t*>(smem + m.o_gtab);
  uint8_t* gops = reinterpret_cast<uint8_t*>(gpoff + g.n_ops);
  uint8_t* glc = gops + g.n_ops;
  uint8_t* grc = glc + g.n_ops;
  const int off = a.out_off[p];
  for (int c = tid; c < g.n_prm; c += 256) {
    hp.z[c] = q.z[off + c];
    hp.cls[c] = q.cls[off + c];
    hp.smap[c] = a.gmap[g.prm_off + c] | ((int)q.rule[g.prm_off + c] << 16);
  }
  for (int i = tid; i < 3 * q.C; i += 256) hp.tf[i] = q.tf[i];
  for (int i = tid; i < 3; i += 256) gprm[g.n_prm + i] = 0.0;      // (the tail padding the reverse pass may read)
  for (int i = tid; i < g.n_ops; i += 256) {
    gpoff[i] = a.gpoff[g.node_off + i];
    gops[i] = a.gops[g.node_off + i]; glc[i] = a.glc[g.node_off + i]; grc[i] = a.grc[g.node_off + i];
  }
  if (tid == 0) hp.st[HMC_ST_ZN] = q.z_noise[p];
  if (q.out_trace != nullptr)
    for (int i = tid; i < 4 * q.n_hmc; i += 256) q.out_trace[(long long)p * 4 * q.n_hmc + i] = __builtin_nan("");
  __syncthreads();
  if (tid == 0) {
    HmcCtl hc;
    for (int c = 0; c < g.n_prm; ++c) hc.nsel += hp.cls[c] >= 0 ? 1 : 0;
    *hmc_ctl_ptr(smem, m) = hc;
  }
}

// The device "recompile" in front of every evaluation: z -> theta (the caller-order vector), noise; the value program's parameters
// through the slot map by emit's own operations (agp_engine.hip: 1 / (l l), 1 / l, -2 / (l l), pi / p — IEEE division), the gradient
// program's parameters and its moving-leaf flags; the right-hand side, which the forward solve consumes.  Ends behind a barrier.
__device__ __forceinline__ void series_hmc_recompile(const SeriesHmcArgs& a, int p, const SeriesHmcLds& m, double* smem, int n, long long o0) {
  const int tid = threadIdx.x;
  const SeriesHmcParams& q = *a.hm;
  const GProgHdr g = a.ghdr[p];
  const HmcLds hp = hmc_lds_ptrs(smem, m);
  double* prm = smem + m.o_prm;
  double* gprm = smem + m.o_gprm;
  const int32_t* gpoff = reinterpret_cast<const int32_t*>(smem + m.o_gtab);
  const uint8_t* gops = reinterpret_cast<const uint8_t*>(gpoff + g.n_ops);
  uint8_t* gmv = const_cast<uint8_t*>(gops) + 3 * g.n_ops;
  for (int c = tid; c < g.n_prm; c += 256) hp.th[c] = hp.cls[c] < 0 ? hp.z[c] : hmc_transform(hp.tf, hp.cls[c], hp.z[c]);
  if (tid == 0) hp.st[HMC_ST_NOISE] = hmc_transform(hp.tf, q.noise_class, hp.st[HMC_ST_ZN]) + q.noise_jitter;
  if (tid < m.np) {
    smem[m.o_rvec + tid] = tid < n ? a.xs[o0 + tid] : 0.0;
    smem[m.o_avec + tid] = 0.0;
  }
  __syncthreads();
  for (int i = tid; i < g.n_ops; i += 256) {
    const int o = gops[i], po = gpoff[i];
    const int k = prm_count(o);
    for (int j = 0; j < k; ++j) {
      const int s = hp.smap[po + j];
      const double v = hp.th[s & 0xffff];
      gprm[po + j] = v;
      prm[po + j] = hmc_rule_apply(s >> 16, v);
    }
    const bool stat = (o == OP_SE || o == OP_GE || o == OP_PER);
    gmv[i] = (stat && gprm[po + (o == OP_SE ? 1 : 2)] != 0.0) ? 1 : 0;
  }
  __syncthreads();
}

// The final state and the counts of particle p (every exit of the chain)
__device__ __forceinline__ void series_hmc_write(const SeriesHmcArgs& a, int p, const HmcLds& hp, const HmcCtl& hc, int npc) {
  const int tid = threadIdx.x;
  const SeriesHmcParams& q = *a.hm;
  const int off = a.out_off[p];
  for (int c = tid; c < npc; c += 256) { q.out_z[off + c] = hp.z[c]; q.out_prm[off + c] = hp.th[c]; }
  if (tid == 0) {
    q.out_z_noise[p] = hp.st[HMC_ST_ZN];
    q.out_noise[p] = hp.st[HMC_ST_NOISE];
    for (int k = 0; k < 4; ++k) q.out_counts[4 * p + k] = hc.cnt[k];
  }
}

// Between two evaluations: what the one that has just finished (hc.ph) means for the chain, in every thread alike — the decisions
// are functions of LDS values every thread reads in the same order; the per-coordinate work is one thread per coordinate.  Returns
// true when another evaluation (of kind hc.mode, at the state now in LDS) is wanted, false when the particle is done and written.
// One move is Gen.hmc taken literally: an evaluation at the current state, momenta, L leapfrog steps with an evaluation each,
// alpha = (U_new - U_0) + (K_new - K_0), accept iff log u < alpha.  Randomness: Philox block (c0, iteration, move, HMC_PHILOX_TAG)
// under the key (seeds[p], 0): momentum k of the selection (caller order) is word k % 4 of block c0 = k / 4; u is word 0 of c0 = 2^32.
__device__ __forceinline__ bool series_hmc_ctl(const SeriesHmcArgs& a, int p, const HmcLds& hp, int npc) {
  const int tid = threadIdx.x;
  const SeriesHmcParams& q = *a.hm;
  HmcCtl* const ctl = reinterpret_cast<HmcCtl*>(hp.st + HMC_ST_CTL);
  __syncthreads();      // the evaluation's results: st[LP], st[BAD], grd, st[GN]
  HmcCtl hc = *ctl;
  // every thread carries the same control state; thread 0 puts it back, once every thread has read it
  auto again = [&]() { __syncthreads(); if (tid == 0) *ctl = hc; return true; };
  const bool bad = hp.st[HMC_ST_BAD] != 0.0;
  const unsigned long long seed = q.seeds[p];
  const bool nz = hc.mv == 1;      // the noise move: z_noise alone
  const double ninf = -__builtin_inf();
  if (hc.ph == HMC_PH_FINAL || (hc.ph == HMC_PH_INIT && bad)) {
    series_hmc_write(a, p, hp, hc, npc);
    return false;
  }
  if (hc.ph != HMC_PH_INIT) {
    // ---- the gradient in z: -z_i + (d logpdf / d theta_i) (d theta_i / d z_i), in place ----
    if (!bad) {
      if (!nz) {
        for (int c = tid; c < npc; c += 256)
          hp.grd[c] = hp.cls[c] >= 0 ? fma(hp.grd[c], hmc_dtheta(hp.tf, hp.cls[c], hp.th[c]), -hp.z[c]) : 0.0;
      } else if (tid == 0) {
        hp.st[HMC_ST_GZN] = fma(hp.st[HMC_ST_GN], hmc_dtheta(hp.tf, q.noise_class, hp.st[HMC_ST_NOISE] - q.noise_jitter), -hp.st[HMC_ST_ZN]);
      }
    }
    __syncthreads();
    bool ok = !bad && isfinite(hp.st[HMC_ST_LP]) && isfinite(hp.st[HMC_ST_NOISE]);
    double zz = 0.0;
    if (ok) {
      for (int c = 0; c < npc; ++c) ok = ok && isfinite(hp.th[c]);
      if (!nz) {
        for (int c = 0; c < npc; ++c)
          if (hp.cls[c] >= 0) { ok = ok && isfinite(hp.grd[c]); zz = fma(hp.z[c], hp.z[c], zz); }
      } else {
        ok = ok && isfinite(hp.st[HMC_ST_GZN]);
        zz = hp.st[HMC_ST_ZN] * hp.st[HMC_ST_ZN];
      }
    }
    const double U = hp.st[HMC_ST_LP] - 0.5 * zz;
    __syncthreads();      // (every thread has read what the updates below overwrite)
    const double he = 0.5 * hc.eps;
    bool finish = false, accept = false;
    double alpha = ninf;
    if (hc.ph == HMC_PH_START) {
      hc.logu = log(philox_uniform(philox4x64_10(1ull << 32, (uint64_t)hc.it, (uint64_t)hc.mv, HMC_PHILOX_TAG, seed, 0).w[0]));
      if (!ok) {
        finish = true;
      } else {
        hc.U0 = U;
        if (!nz) {
          for (int c = tid; c < npc; c += 256)
            if (hp.cls[c] >= 0) {
              int k = 0;
              for (int j = 0; j < c; ++j) k += hp.cls[j] >= 0 ? 1 : 0;
              const Philox4 b = philox4x64_10((uint64_t)(k >> 2), (uint64_t)hc.it, 0, HMC_PHILOX_TAG, seed, 0);
              hp.mom[c] = ndtri(philox_uniform(b.w[k & 3]));
              hp.zs[c] = hp.z[c];
            }
        } else if (tid == 0) {
          hp.st[HMC_ST_MN] = ndtri(philox_uniform(philox4x64_10(0, (uint64_t)hc.it, 1, HMC_PHILOX_TAG, seed, 0).w[0]));
          hp.st[HMC_ST_ZSN] = hp.st[HMC_ST_ZN];
        }
        __syncthreads();
        double mm = 0.0;
        if (!nz) { for (int c = 0; c < npc; ++c) if (hp.cls[c] >= 0) mm = fma(hp.mom[c], hp.mom[c], mm); }
        else mm = hp.st[HMC_ST_MN] * hp.st[HMC_ST_MN];
        hc.K0 = -0.5 * mm;
        __syncthreads();
        if (hc.L == 0) {      // (no leapfrog step: the state stands, alpha = 0)
          finish = true; alpha = 0.0; accept = hc.logu < alpha;
        } else {
          if (!nz) {
            for (int c = tid; c < npc; c += 256)
              if (hp.cls[c] >= 0) { hp.mom[c] = fma(he, hp.grd[c], hp.mom[c]); hp.z[c] = fma(hc.eps, hp.mom[c], hp.z[c]); }
          } else if (tid == 0) {
            hp.st[HMC_ST_MN] = fma(he, hp.st[HMC_ST_GZN], hp.st[HMC_ST_MN]);
            hp.st[HMC_ST_ZN] = fma(hc.eps, hp.st[HMC_ST_MN], hp.st[HMC_ST_ZN]);
          }
          hc.step = 1; hc.ph = HMC_PH_LEAP;
          return again();
        }
      }
    } else {      // HMC_PH_LEAP: the evaluation at the end of leapfrog step hc.step
      if (ok) {
        const bool more = hc.step < hc.L;
        if (!nz) {
          for (int c = tid; c < npc; c += 256)
            if (hp.cls[c] >= 0) {
              double mo = fma(he, hp.grd[c], hp.mom[c]);
              if (more) { mo = fma(he, hp.grd[c], mo); hp.z[c] = fma(hc.eps, mo, hp.z[c]); }
              hp.mom[c] = mo;
            }
        } else if (tid == 0) {
          double mo = fma(he, hp.st[HMC_ST_GZN], hp.st[HMC_ST_MN]);
          if (more) { mo = fma(he, hp.st[HMC_ST_GZN], mo); hp.st[HMC_ST_ZN] = fma(hc.eps, mo, hp.st[HMC_ST_ZN]); }
          hp.st[HMC_ST_MN] = mo;
        }
        if (more) { ++hc.step; return again(); }
        __syncthreads();
        double mm = 0.0;
        if (!nz) { for (int c = 0; c < npc; ++c) if (hp.cls[c] >= 0) mm = fma(hp.mom[c], hp.mom[c], mm); }
        else mm = hp.st[HMC_ST_MN] * hp.st[HMC_ST_MN];
        alpha = (U - hc.U0) + (-0.5 * mm - hc.K0);
        accept = hc.logu < alpha;
      }
      finish = true;
      if (!accept) {      // back to the saved state (a trajectory that left the positive definite region included)
        if (!nz) { for (int c = tid; c < npc; c += 256) if (hp.cls[c] >= 0) hp.z[c] = hp.zs[c]; }
        else if (tid == 0) hp.st[HMC_ST_ZN] = hp.st[HMC_ST_ZSN];
      }
    }
    // ---- the move is over ----
    if (finish) {
      hc.moved = 1;
      if (!ok) ++hc.cnt[3];
      if (!nz) { ++hc.cnt[1]; hc.cnt[0] += accept ? 1 : 0; hc.pacc = accept ? 1 : 0; hc.pmade = 1; }
      else hc.cnt[2] += accept ? 1 : 0;
      if (q.out_trace != nullptr) {
        const int e = (hc.it * 2 + hc.mv) * 2;      // (the thread that set the entry to NaN writes it)
        double* t = q.out_trace + (long long)p * 4 * q.n_hmc;
        if (tid == (e & 255)) t[e] = alpha;
        if (tid == ((e + 1) & 255)) t[e + 1] = hc.logu;
      }
    }
  }
  // ---- the next move: parameters, then noise, then the exit check of the iteration ----
  int it = hc.it, mv = hc.ph == HMC_PH_INIT ? 0 : hc.mv + 1;
  for (;;) {
    if (mv == 2) {
      if (hc.pmade) {
        hc.nrej = hc.pacc ? 0 : hc.nrej + 1;
        if (q.n_exit > 0 && hc.nrej >= q.n_exit) hc.stop = 1;
      }
      hc.pmade = 0; ++it; mv = 0;
    }
    if (it >= q.n_hmc || hc.stop) {
      if (!hc.moved) {      // no move was made: the first evaluation is the final one
        series_hmc_write(a, p, hp, hc, npc);
        return false;
      }
      hc.ph = HMC_PH_FINAL; hc.mode = HMC_EV_VALUE;
      return again();
    }
    if (mv == 0 && hc.nsel == 0) { mv = 1; continue; }
    if (mv == 1 && q.L_noise == 0) { mv = 2; continue; }
    break;
  }
  hc.it = it; hc.mv = mv; hc.ph = HMC_PH_START; hc.step = 0;
  hc.L = mv == 0 ? q.L_prm : q.L_noise;
  hc.eps = mv == 0 ? q.eps_prm : q.eps_noise;
  hc.mode = (mv == 0 || (q.flags & HMC_FLAG_FULL_NOISE_GRAD)) ? HMC_EV_GRAD : HMC_EV_GNOISE;
  return again();
}

// The body of every instantiation: stages 1-5 (value kernel, probe, gradient kernel, predictive kernel alike — the same statements),
// with GS > 0 (gradient tape of GS nodes) the stages G1-G5 behind them, with SeriesPredArgs or SeriesSumArgs the stages P1-P2.
// With SeriesHmcArgs the statements from stage 2 to G5 are the body of a loop (two labels and their gotos, which only that
// instantiation has: the other instantiations' statements stand where they stood): series_hmc_recompile in front of stage 2,
// series_hmc_ctl behind G5, G5 reducing into LDS.
template <int D, bool PROBE, int GS, class ArgsT>
__device__ __forceinline__ void series_body(const ArgsT& a, double* smem) {
  constexpr int E = 4;
  constexpr bool SUM = std::is_same_v<ArgsT, SeriesSumArgs>;         // the decomposition twin: composite programs, coded query rows
  constexpr bool PRED = std::is_same_v<ArgsT, SeriesPredArgs> || SUM;    // the predictive branches (P1, P2, series_pred_lds) are shared
  constexpr bool PROBA = std::is_same_v<ArgsT, SeriesProbaArgs>;      // the held-out twin: n below is the JOINT length
  constexpr bool SAMPLE = std::is_same_v<ArgsT, SeriesSampleArgs>;    // the sampling twin: the same, the query rows' right-hand side 0
  constexpr bool JOINT = PROBA || SAMPLE;
  constexpr bool HMC = std::is_same_v<ArgsT, SeriesHmcArgs>;          // the HMC twin: stages 2 .. G5 in a loop, the chain between them
  int tid = threadIdx.x, l = tid & 63, w = tid >> 6, l15 = l & 15, lq = l >> 4;      // (constant but for the HMC twin's hmc_eval)
  int p, n;
  long long o0 = 0;
  [[maybe_unused]] int ntr = 0;            // JOINT: training points (rows [ntr, n) are the query rows)
  [[maybe_unused]] long long q0 = 0;       // JOINT: the series' first query
  if constexpr (PROBE) {
    p = blockIdx.x;
    n = a.n;
  } else {
    p = a.wg[blockIdx.x];
    const int sidx = a.series[p];
    o0 = a.pt_off[sidx];
    n = (int)(a.pt_off[sidx + 1] - o0);
    if constexpr (JOINT) {
      q0 = a.q_off[sidx];
      const long long mq = a.q_off[sidx + 1] - q0;
      ntr = n;
      n = (mq <= 0 || mq > SERIES_MAX_N) ? 0 : n + (int)mq;      // (nothing held out: never launched, like an empty series)
    }
  }
  if (n <= 0 || n > SERIES_MAX_N) {      // (the host answers empty series itself and refuses long ones: never launched ...
    if constexpr (SUM) {                 // ... but for the prior predictive of an empty series)
      const int rb = n == 0 ? series_prior_predict_sum<D>(a, p, smem) : 0;
      if (tid == 0) { a.out_lp[p] = 0.0; a.out_info[p] = rb; }
      return;
    } else if constexpr (PRED) {
      if (n == 0) series_prior_predict<D>(a, p, smem);
    }
    if (tid == 0) { a.out_lp[p] = 0.0; a.out_info[p] = 0; }
    return;
  }
  const ProgHdr h = [&]() -> ProgHdr { if constexpr (PROBE) return ProgHdr{}; else return a.hdr[p]; }();
  const auto m = [&]() {
    if constexpr (HMC) return series_hmc_lds(n, h.n_ops, h.n_prm, h.n_cp, a.ghdr[p].n_ops, a.ghdr[p].n_prm, a.C);
    else if constexpr (GS > 0) return series_grad_lds(n, h.n_ops, h.n_prm, h.n_cp, a.ghdr[p].n_ops, a.ghdr[p].n_prm);
    else if constexpr (PRED) return series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp);
    else return series_lds(n, h.n_ops, h.n_prm, h.n_cp);
  }();
  const int nb = m.nb, np = m.np;
  double* Wl = smem;
  [[maybe_unused]] double* tpt = smem + m.o_tpt;      // (tpt, etab, prm, ops, sig: unused by the probe, whose map has none of them)
  double* rvec = smem + m.o_rvec;
  double* avec = smem + m.o_avec;
  [[maybe_unused]] double* etab = smem + m.o_etab;
  [[maybe_unused]] double* prm = smem + m.o_prm;
  [[maybe_unused]] int* ops = reinterpret_cast<int*>(smem + m.o_ops);
  [[maybe_unused]] double* sig = smem + m.o_sig;
  double* sm = smem + m.o_blk;

  if constexpr (PROBE) {
    // ---- 1. - 3. replaced: the caller's right-hand side and the lower triangle of the caller's matrix, block layout as below ----
    if (tid < np) {
      rvec[tid] = (tid < n && a.y != nullptr) ? a.y[(long long)p * n + tid] : 0.0;
      avec[tid] = 0.0;
    }
    const double* Kp = a.K + (long long)p * n * n;
    const int nblk = nb * (nb + 1) / 2;
    for (int b = w; b < nblk; b += 4) {
      int rb, cb;
      series_blk_rc(b, rb, cb);
      double* blk = sm + blk_idx(rb, cb) * 256;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int ri = rb * 16 + l15, ci = cb * 16 + lq + 4 * e;
        const int hi = ri > ci ? ri : ci, lo = ri > ci ? ci : ri;      // (a diagonal block holds both triangles, as cov_finalize leaves it)
        blk[64 * e + l] = hi < n ? Kp[(long long)hi * n + lo] : (ri == ci ? 1.0 : 0.0);
      }
    }
  } else {
    // ---- 1. inputs ----
    if constexpr (JOINT) {
      // the joint points: the series' times, then — directly behind them, no padding between — its query times; xs, then the held-out values
      if (tid < np) {
        const int k = tid < n ? tid : n - 1;
        tpt[tid] = k < ntr ? a.ts[o0 + k] : a.ts_pred[q0 + (k - ntr)];
        if constexpr (SAMPLE) rvec[tid] = tid < ntr ? a.xs[o0 + tid] : 0.0;
        else rvec[tid] = tid < ntr ? a.xs[o0 + tid] : tid < n ? a.y_pred[q0 + (tid - ntr)] : 0.0;
        avec[tid] = 0.0;
      }
    } else if (tid < np) {
      tpt[tid] = a.ts[o0 + (tid < n ? tid : n - 1)];      // (padding points: a finite time; their entries are overwritten with identity)
      rvec[tid] = tid < n ? a.xs[o0 + tid] : 0.0;
      avec[tid] = 0.0;
    }
    if (AGP_EXP_TABLE && tid < AGP_EXP_TAB_N) etab[tid] = fm::c_exp_tab[tid];
    for (int i = tid; i < h.n_prm + 2; i += 256) prm[i] = a.prm[h.prm_off + i];      // (the parameter buffer carries two doubles of tail padding)
    for (int i = tid; i < h.n_ops; i += 256) ops[i] = (int)a.ops[h.op_off + i];
    __syncthreads();
    if constexpr (HMC) series_hmc_stage(a, p, m, smem);
  }
hmc_eval: __attribute__((unused));      // HMC: every evaluation of the chain starts here, at the state in LDS (a label cannot stand
  if constexpr (!PROBE) {               // inside a constexpr if: the production branch is closed in front of it and opened again)
    if constexpr (HMC) {
      // (the thread's indices are formed again for every evaluation: what follows from them — the addresses of every stage — is
      // then computed where it is used, as in the gradient kernel, not kept in registers around the whole loop)
      asm volatile("" : "+v"(tid));
      l = tid & 63; w = tid >> 6; l15 = l & 15; lq = l >> 4;
      series_hmc_recompile(a, p, m, smem, n, o0);
    }

    // ---- 2. per-point tables (cov_prologue's arithmetic) ----
    if (h.n_cp > 0) {
      if (tid < np) series_sigma_cp<SUM>(h, ops, prm, sig, tid, tpt[tid]);      // (SUM: training points are the observable, code 0)
      __syncthreads();
    }

    // ---- 3. K + noise I, lower block triangle; one block per wave and pass, lane (i = l%16, q = l/16) <-> elements (i, q + 4 e) ----
    {
      const double noise = [&]() { if constexpr (HMC) return smem[m.o_st + HMC_ST_NOISE]; else return a.noise[p]; }();
      [[maybe_unused]] double noise_q = 0.0;      // JOINT: the diagonal addend of the query rows
      if constexpr (JOINT) noise_q = a.noise_pred[p];
      const int nblk = nb * (nb + 1) / 2;
      for (int b = w; b < nblk; b += 4) {
        int rb, cb;
        series_blk_rc(b, rb, cb);
        double tr[E], tc[E], out[E], lt[E];
        int ri[E], ci[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          ri[e] = rb * 16 + l15;
          ci[e] = cb * 16 + lq + 4 * e;
          tr[e] = tpt[ri[e]];
          tc[e] = tpt[ci[e]];
          lt[e] = 0.0;
        }
        eval_program<D, E, 0>(h, ops, prm, sig, tr, tc, ri, ci, lt, out, etab);
        double* blk = sm + blk_idx(rb, cb) * 256;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if constexpr (JOINT) blk[64 * e + l] = cov_finalize(out[e], ri[e], ci[e], n, np, 0, ri[e] < ntr ? noise : noise_q);
          else blk[64 * e + l] = cov_finalize(out[e], ri[e], ci[e], n, np, 0, noise);
        }
      }
    }
  }
  __syncthreads();

  // ---- 4. + 5. factorisation with the forward solve carried along: the block steps of factor_diag_tile over nb block rows
  //      (lds_chol_steps, agp_lds_chol.hpp); r_ib -= L(ib,jb) alpha_jb on one thread per row of waves 1 .. 3 (192 >= np) ----
  int bad = 0;           // first non-positive pivot (1-based index in the series), 0 = none; kept by wave 0
  lds_chol_steps<0>(sm, Wl, rvec, avec, nb, nb, 64, np, 0, bad, tid);

  // ---- the value: 2 sum log L_ii (padding rows: log 1) and alpha'alpha, reduced in a fixed order
  //      (JOINT: both over the query rows [ntr, n) alone — the conditional density of the held-out values) ----
  [[maybe_unused]] double lgd = 0.0;      // JOINT: log L_kk of the thread's own row
  {
    double ld = 0.0;
    if (tid < np) {
      const double dii = sm[blk_idx(tid >> 4, tid >> 4) * 256 + 17 * (tid & 15)];
      if constexpr (JOINT) {
        lgd = log(dii);
        ld = tid >= ntr ? 2.0 * lgd : 0.0;
      } else {
        ld = 2.0 * log(dii);
      }
    }
    Wl[tid] = ld;      // (the last inverse block has been consumed)
    if constexpr (JOINT) {
      if (tid == 0) rvec[0] = (double)bad;      // (wave 0 keeps the first bad pivot; rvec is dead)
    }
  }
  __syncthreads();
  if (w == 0) {
    double ld = (Wl[l] + Wl[l + 64]) + (Wl[l + 128] + Wl[l + 192]);
    double ss = 0.0;
    if constexpr (JOINT) {
      for (int i = l; i < np; i += 64) ss = i >= ntr ? fma(avec[i], avec[i], ss) : ss;
    } else {
      for (int i = l; i < np; i += 64) ss = fma(avec[i], avec[i], ss);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ss += __shfl_xor(ss, off); ld += __shfl_xor(ld, off); }
    if (l == 0) {
      double lp;
      if constexpr (JOINT) {      // m log 2 pi, and the Jacobian of the series' own transform: m log|slope|
        const double mq = (double)(n - ntr);
        lp = -0.5 * (mq * 1.8378770664093454835606594728112 + ld + ss) + mq * log(fabs(a.y_slope[a.series[p]]));
      } else if constexpr (HMC) {
        // (the statement below, written as the fused operation it compiles to in the other instantiations: in a loop the compiler
        // forms the invariant product n log 2 pi once, in front of it, and the sum is then rounded twice — out_logpdf would differ
        // from the value entry's in the last bit; tests/test_gpu_series_hmc.py compares the bits)
        lp = -0.5 * (fma((double)n, 1.8378770664093454835606594728112, ld) + ss);
      } else {
        lp = -0.5 * ((double)n * 1.8378770664093454835606594728112 + ld + ss);
      }
      // (the sampling twin has no density to report — its query right-hand side is 0 — and its entry never reads out_lp: without the
      // store the two reductions above are dead code in that instantiation)
      if constexpr (!SAMPLE) a.out_lp[p] = bad != 0 ? __builtin_nan("") : lp;
      a.out_info[p] = bad;
      if constexpr (HMC) { smem[m.o_st + HMC_ST_LP] = lp; smem[m.o_st + HMC_ST_BAD] = (double)bad; }
      if constexpr (PROBE) { a.out_part[2 * p] = ld; a.out_part[2 * p + 1] = ss; }
    }
  }
  if constexpr (PROBE) {      // the factor as stages 4 and 5 left it: packed blocks (diagonal blocks: zero above the diagonal) and alpha
    const int nel = nb * (nb + 1) / 2 * 256;
    for (int i = tid; i < nel; i += 256) a.out_blk[(long long)p * nel + i] = sm[i];
    if (tid < np) a.out_alpha[(long long)p * np + tid] = avec[tid];
  }

  if constexpr (PROBA) {
    // ---- the per-point terms: log N(y_j | training data, y_0 .. y_{j-1}) from row ntr + j of the joint factor (chain rule) ----
    if (a.out_terms != nullptr && tid >= ntr && tid < n) {
      const double z = avec[tid];
      const double t = (-0.5 * fma(z, z, 1.8378770664093454835606594728112) - lgd) + log(fabs(a.y_slope[a.series[p]]));
      a.out_terms[a.out_off[p] + (tid - ntr)] = rvec[0] != 0.0 ? __builtin_nan("") : t;
    }
  }

  if constexpr (SAMPLE) {
    // ================= sampling: rows [ntr, n) of the factor read out (tpt is dead: it takes mu*) =================
    series_sample_readout(a, p, sm, avec, tpt, rvec[0] != 0.0, ntr, n - ntr);
  }

  if constexpr (PRED) {
    // ================= prediction: mean = K21 K11^-1 x = VT beta, var = diag(K22) - rowsums(VT^2) + noise_pred, VT = K21 L^-T =================
    // LDS now: as the gradient finds it — L in the packed blocks, beta in avec (padding: 0), tpt, the program and its tables.
    const int sidx = a.series[p];
    const long long q0 = a.q_off[sidx];
    const int mq = (int)(a.q_off[sidx + 1] - q0);
    if (mq <= 0) return;
    double* om = a.out_mean + a.out_off[p];
    double* ov = a.out_var + a.out_off[p];
    if (tid == 0) rvec[0] = (double)bad;      // (wave 0 keeps the first bad pivot; rvec is dead)
    [[maybe_unused]] int* rowbad = reinterpret_cast<int*>(Wl);      // SUM: the first row without a raw marginal (Wl is dead: this
    if constexpr (SUM) {                                            // thread's wave has read the value's reduction out of it)
      if (tid == 0) *rowbad = 0x7fffffff;
    }
    // ---- P1. the diagonal blocks L(i,i)^-T in place (G1's statements; the log-det has been read) ----
    series_diag_inv_t(sm, nb, w, l);
    __syncthreads();
    if constexpr (SUM) {
      if (rvec[0] != 0.0) {      // a bad pivot: NaN in all of the particle's outputs, info stays the pivot
        const int rows = (a.M + 1) * mq;
        double* ox = a.out_x + (long long)a.nq * a.out_off[p];
        for (int g = tid; g < rows; g += 256) { om[g] = __builtin_nan(""); ov[g] = __builtin_nan(""); }
        for (long long i = tid; i < (long long)rows * a.nq; i += 256) ox[i] = __builtin_nan("");
        return;
      }
      // ---- P2 on the (M + 1) mq coded rows, read out in the same lanes; a failed row marks the particle: info = n + g + 1 ----
      const int rb = series_sum_rows<D>(a, p, h, ops, prm, sig, tpt, avec, etab, sm, n, nb, q0, mq, rowbad);
      if (rb != 0 && tid == 0) a.out_info[p] = n + rb;
      return;
    } else {
      if (rvec[0] != 0.0) {      // a bad pivot: NaN in the particle's whole block (the value is NaN already), nothing else
        for (int q = tid; q < mq; q += 256) { om[q] = __builtin_nan(""); ov[q] = __builtin_nan(""); }
        return;
      }
      // ---- P2. query blocks, wave by wave ----
      series_predict_blocks<D>(h, ops, prm, sig, tpt, avec, etab, sm, n, nb, a.ts_pred + q0, mq, a.noise_pred[p], om, ov);
    }
  }

  if constexpr (GS > 0) {
    // ================= gradient: d logpdf / d theta = sum_ab G_ab dK_ab / d theta, G = 1/2 (alpha alpha' - K^-1); d / d noise = tr G =================
    // LDS now: L in the packed blocks (diagonal blocks: zero above the diagonal; rows / columns past n: identity), beta = L^-1 x in
    // avec (padding: 0), tpt.  rvec and Wl are dead.
    const GProgHdr g = a.ghdr[p];
    double* alpha = smem + m.o_alpha;
    double* gprm = smem + m.o_gprm;
    int32_t* gpoff = reinterpret_cast<int32_t*>(smem + m.o_gtab);
    uint8_t* gops = reinterpret_cast<uint8_t*>(gpoff + g.n_ops);
    uint8_t* glc = gops + g.n_ops;
    uint8_t* grc = glc + g.n_ops;
    uint8_t* gmv = grc + g.n_ops;      // 1: stationary leaf with non-zero amplitude (see grad_elements)
    double* red = smem + m.o_red;
    if (tid == 0) rvec[0] = (double)bad;      // (wave 0 keeps the first bad pivot)
    // the gradient program (k_grad_contract's staging; HMC: series_hmc_stage and series_hmc_recompile have done it)
    if constexpr (!HMC) {
      for (int i = tid; i < g.n_prm + 3; i += 256) gprm[i] = a.gprm[g.prm_off + i];
      for (int i = tid; i < g.n_ops; i += 256) {
        const int po = a.gpoff[g.node_off + i];
        const int o = a.gops[g.node_off + i];
        gpoff[i] = po;
        gops[i] = (uint8_t)o; glc[i] = a.glc[g.node_off + i]; grc[i] = a.grc[g.node_off + i];
        const bool stat = (o == OP_SE || o == OP_GE || o == OP_PER);
        gmv[i] = (stat && a.gprm[g.prm_off + po + (o == OP_SE ? 1 : 2)] != 0.0) ? 1 : 0;
      }
    }
    __syncthreads();
    if constexpr (HMC) {       // a bad pivot, or the value alone is wanted: the chain decides what follows
      if (rvec[0] != 0.0 || hmc_ctl_ptr(smem, m)->mode == HMC_EV_VALUE) goto hmc_ctl;
    } else if (rvec[0] != 0.0) {      // a bad pivot: NaN in the whole gradient block and d / d noise (the value is NaN already), nothing else
      for (int q = tid; q < g.n_prm; q += 256) a.out_grad[a.out_off[p] + a.gmap[g.prm_off + q]] = __builtin_nan("");
      if (tid == 0) a.out_gnoise[p] = __builtin_nan("");
      return;
    }
    // per-point tables in the gradient program's node order (the order grad_elements counts ChangePoint nodes in), same arithmetic
    // as stage 2, each followed — n_cp tables on — by its complement 1 - sigma (the map's csig, directly behind sig)
    if (g.n_cp > 0 && tid < np) {
      const double t = tpt[tid];
      int c = 0;
      for (int ip = 0; ip < g.n_ops; ++ip)
        if (gops[ip] == OP_CP) {
          const double* q = gprm + gpoff[ip];
          const double th = tanh((q[0] - t) / q[1]);
          sig[c * 256 + tid] = 0.5 * (1.0 + th);
          sig[(g.n_cp + c) * 256 + tid] = 0.5 * (1.0 - th);      // 1 - sigma from the same tanh: exact where sigma is near 1 (grad_elements, CSIG)
          ++c;
        }
    }
    // ---- G1. Z = L^-T in place, block Z(j,i) (j <= i) in the slot of lower block (i,j), column-major: K^-1 = Z Z' then contracts
    //      over natural (conflict-free) LDS reads exactly like L L' does.  First the diagonal: Z(i,i) = L(i,i)^-T, one block per wave
    //      and pass, column c of L(i,i)^-1 by forward substitution in lane c (the reads of L are broadcasts) ----
    series_diag_inv_t(sm, nb, w, l);
    __syncthreads();
    // ---- G2. column i of Z (slot row i): Z(j,i) = -[sum_{k=j}^{i-1} Z(j,k) L(i,k)'] L(i,i)^-T, j < i.  Reads row i of L (slots (i,k))
    //      and finished columns k < i of Z (slots (k,j)); its results replace row i of L, so they wait in registers until every
    //      wave has read that row: blocks j = w, w + 4, w + 8 per wave (nb <= 11: at most three) ----
    for (int i = 1; i < nb; ++i) {
      d4 res[3];
      double fw[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) fw[s4] = sm[blk_idx(i, i) * 256 + l15 * 16 + 4 * s4 + lq];      // L(i,i)^-1 (l15, 4 s4 + lq) = Z(i,i)'
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int j = w + 4 * u;
        res[u] = d4{0.0, 0.0, 0.0, 0.0};
        if (j < i) {
          d4 acc = d4{0.0, 0.0, 0.0, 0.0};
          for (int k = j; k < i; ++k) {
            const double* lb = sm + blk_idx(i, k) * 256;
            const double* zb = sm + blk_idx(k, j) * 256;
            double fa[4], fb[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) { fa[s4] = lb[64 * s4 + l]; fb[s4] = zb[64 * s4 + l]; }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) acc = mfma(fa[s4], fb[s4], acc);      // += Z(j,k) L(i,k)'
          }
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) res[u] = mfma(fw[s4], -acc[s4], res[u]);      // (-C) L(i,i)^-T
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int j = w + 4 * u;
        if (j < i) {
          double* blk = sm + blk_idx(i, j) * 256;
#pragma unroll
          for (int r = 0; r < 4; ++r) blk[64 * r + l] = res[u][r];
        }
      }
      __syncthreads();
    }
    // ---- G3. alpha = Z beta: one row per thread, columns in ascending order ----
    if (tid < np) {
      const int j = tid >> 4, r = tid & 15;
      double s = 0.0;
      for (int k = j; k < nb; ++k) {
        const double* zb = sm + blk_idx(k, j) * 256;
#pragma unroll
        for (int c = 0; c < 16; ++c) s = fma(zb[c * 16 + r], avec[k * 16 + c], s);
      }
      alpha[tid] = s;
    }
    __syncthreads();
    // ---- G4. contraction, K^-1 never stored: lower block (rb, cb) -> wave b % 4 (b its row-major index: a function of nb alone) forms
    //      K^-1(rb,cb) = sum_{k >= rb} Z(rb,k) Z(cb,k)' in registers — lane (i = l%16, q = l/16) <-> elements (i, q + 4 e), the map of
    //      stage 3 — turns it into G and runs the reverse-mode pass on its four elements.  Off-diagonal blocks stand for their mirror
    //      image (weight 2); diagonal blocks are evaluated in full at weight 1; rows / columns past n (identity in Z) weigh 0 ----
    if constexpr (HMC) {
      // a noise move wants d / d noise = tr G = 1/2 (alpha'alpha - tr K^-1) alone, and tr K^-1 = |Z|_F^2 over the rows and columns
      // below n (slot (rb, cb) holds Z(cb, rb): element 64 e + l is row 16 cb + l % 16, column 16 rb + 4 e + l / 16): no MFMA
      // chain, no reverse-mode pass.  Fixed order: thread -> wave -> the four waves, then alpha'alpha in one thread.
      if (hmc_ctl_ptr(smem, m)->mode == HMC_EV_GNOISE) {
        double s2 = 0.0;
        const int nblk = nb * (nb + 1) / 2;
        for (int b = w; b < nblk; b += 4) {
          int rb, cb;
          series_blk_rc(b, rb, cb);
          const double* zb = sm + blk_idx(rb, cb) * 256;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const double v = zb[64 * e + l];
            s2 = (cb * 16 + l15 < n && rb * 16 + 4 * e + lq < n) ? fma(v, v, s2) : s2;
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s2 += __shfl_xor(s2, off);
        if (l == 0) red[w] = s2;
        __syncthreads();
        if (tid == 0) {
          double aa = 0.0;
          for (int i = 0; i < n; ++i) aa = fma(alpha[i], alpha[i], aa);
          smem[m.o_st + HMC_ST_GN] = 0.5 * (aa - (((red[0] + red[1]) + red[2]) + red[3]));
        }
        goto hmc_ctl;
      }
    }
    constexpr int NG = 3 * GS + 2;
    double gacc[NG];
    for (int q = 0; q <= g.n_prm + 2 && q < NG; ++q) gacc[q] = 0.0;
    ScratchAcc<NG> sacc{gacc};
    RegTape<GS, E> tape;
    double gnoise = 0.0;
    {
      const int nblk = nb * (nb + 1) / 2;
      for (int b = w; b < nblk; b += 4) {
        int rb, cb;
        series_blk_rc(b, rb, cb);
        d4 kin = d4{0.0, 0.0, 0.0, 0.0};
        for (int k = rb; k < nb; ++k) {
          const double* za = sm + blk_idx(k, cb) * 256;
          const double* zb = sm + blk_idx(k, rb) * 256;
          double fa[4], fb[4];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) { fa[s4] = za[64 * s4 + l]; fb[s4] = zb[64 * s4 + l]; }
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) kin = mfma(fa[s4], fb[s4], kin);
        }
        const double wfac = rb == cb ? 1.0 : 2.0;
        int ri[E], ci[E];
        double ta[E], tb[E], wg[E], lt[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          ri[e] = rb * 16 + l15;
          ci[e] = cb * 16 + lq + 4 * e;
          const bool valid = ri[e] < n && ci[e] < n;
          const double G = valid ? 0.5 * (alpha[ri[e]] * alpha[ci[e]] - kin[e]) : 0.0;
          if (ri[e] == ci[e]) gnoise += G;
          ta[e] = tpt[ri[e]]; tb[e] = tpt[ci[e]]; wg[e] = wfac * G; lt[e] = 0.0;
        }
        grad_elements<GS, E, true>(g, gops, glc, grc, gmv, gpoff, gprm, sig, ri, ci, ta, tb, wg, lt, false, tape, sacc);
      }
    }
    gacc[g.n_prm] = gnoise;
    // ---- G5. per-thread sums -> lanes of a wave (butterfly) -> the four waves in order -> the caller's parameter order ----
    const int nq = g.n_prm + 1;
    for (int q = 0; q < nq; ++q) {
      double s = gacc[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (l == 0) red[w * nq + q] = s;
    }
    __syncthreads();
    for (int q = tid; q < nq; q += 256) {
      const double s = ((red[q] + red[nq + q]) + red[2 * nq + q]) + red[3 * nq + q];
      if constexpr (HMC) {      // into LDS, the caller's order: the chain reads it
        if (q < g.n_prm) smem[m.o_grd + (reinterpret_cast<const int*>(smem + m.o_cls)[(m.o_tf - m.o_cls) + q] & 0xffff)] = s;
        else smem[m.o_st + HMC_ST_GN] = s;
      } else {
        if (q < g.n_prm) a.out_grad[a.out_off[p] + a.gmap[g.prm_off + q]] = s;
        else a.out_gnoise[p] = s;
      }
    }
  }

hmc_ctl: __attribute__((unused));
  if constexpr (HMC) {
    if (series_hmc_ctl(a, p, hmc_lds_ptrs(smem, m), a.ghdr[p].n_prm)) goto hmc_eval;
  }
}

template <int D, bool PROBE = false>
__global__ __launch_bounds__(256, 2) void k_series_logpdf(std::conditional_t<PROBE, SeriesProbeArgs, SeriesArgs> a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, PROBE, 0>(a, smem);
}

// Value and gradient of one (series, particle) pair by one workgroup: GS = nodes the reverse-mode tape holds (16 or 64; a private
// array, as in k_grad_contract<GS>), D as above.
template <int D, int GS>
__global__ __launch_bounds__(256, 2) void k_series_logpdf_grad(SeriesGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, GS>(a, smem);
}

// rejuvenate_particle_parameters (src/inference_smc_anneal_data.jl:33-76) of one (series, particle) pair by one workgroup: n_hmc
// iterations of an HMC move on the numeric kernel parameters and one on the noise, in the reference's latent space, every
// evaluation the gradient kernel's statements (agp_hmc_series_batch); D and GS as in k_series_logpdf_grad.
template <int D, int GS>
__global__ __launch_bounds__(256, 2) void k_series_hmc(SeriesHmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, GS>(a, smem);
}

// Log-density of one series' held-out values under one particle's predictive by one workgroup: the value kernel's body on the
// joint points (agp_predict_logpdf_series_batch).
template <int D>
__global__ __launch_bounds__(256, 2) void k_series_predict_logpdf(SeriesProbaArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, 0>(a, smem);
}

// Samples, component mean and component covariance of one (series, particle) pair at the series' own query times by one workgroup:
// the held-out twin's factorisation of the joint points, series_sample_readout behind it (agp_predict_sample_series_batch).
template <int D>
__global__ __launch_bounds__(256, 2) void k_series_predict_sample(SeriesSampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, 0>(a, smem);
}

// ... and behind those launches, on the same stream: one workgroup per series; a series with a failed particle (whatever its weight)
// has no valid sample — its whole block of out_x becomes NaN.  Series without query points own nothing (and their particles' info
// words were never written).
#ifndef AGP_SERIES_TEMPLATES_ONLY      // (a plain kernel: defined in ONE unit — agp_kernels_series_hmc.hip includes the templates alone)
__global__ __launch_bounds__(256) void k_series_sample_fill(SeriesSampleFillArgs a) {
  const int s = blockIdx.x;
  const long long q0 = a.q_off[s], m = a.q_off[s + 1] - q0;
  if (m <= 0) return;
  int bad = 0;
  for (long long k = a.pl_off[s] + threadIdx.x; k < a.pl_off[s + 1]; k += 256) bad |= a.info[a.plist[k]] != 0 ? 1 : 0;
  if (!__syncthreads_or(bad)) return;
  double* ox = a.out_x + a.R * q0;
  for (long long i = threadIdx.x; i < a.R * m; i += 256) ox[i] = __builtin_nan("");
}
#endif

// Posterior mean and marginal variance of one (series, particle) pair at the series' own query times by one workgroup, behind the
// value and in the value kernel's LDS (agp_predict_series_batch).
template <int D>
__global__ __launch_bounds__(256, 2) void k_series_predict(SeriesPredArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, 0>(a, smem);
}

// predict_sum's numbers of one (series, particle) pair by one workgroup: the predictive twin on the particle's composite program and
// the (M + 1) m coded rows F_1(T*) .. F_M(T*), X(T*), raw-space marginals and their Normal quantiles read out in the lanes that
// formed them (agp_predict_sum_series_batch).
template <int D>
__global__ __launch_bounds__(256, 2) void k_series_predict_sum(SeriesSumArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  series_body<D, false, 0>(a, smem);
}

}  // namespace agp
