// Long-series value kernel: log N(xs_s; 0, K_p(ts_s) + noise_p I) of one particle on one series of 1 <= n <= LONG_SERIES_MAX_N = 512
// points by ONE workgroup (agp_logpdf_long_series_batch, agp_series.hip) — the value entry of the many-series family above the
// short kernels' cap (agp_series_kernel.hpp: 176 points, where the packed blocks stop fitting into one workgroup's LDS).  At 512
// points the lower triangle of L is 528 blocks of 2 KiB (1.03 MiB): the factor lives in a per-workgroup HBM workspace in the family's
// packed layout — block (rb, cb) column-major at blk_idx(rb, cb) * 256 — and the factorisation runs LEFT-LOOKING by 16-wide block
// columns, so a block is written once, finished, and afterwards only read.
//
// k_long_series_logpdf<D> (256 threads, D = depth of the evaluation stack, 4 or 8), per workgroup:
//   1. ts, xs of the particle's series, its compiled program and parameters -> LDS (series_body's stage 1);
//   2. per-point tables: sigma_cp of every ChangePoint node at all points of the series, LONG_SIG_STRIDE = 512 entries per node
//      (eval_program's SIGSTRIDE; every other kernel keeps its 256);
//   3. per block column j = 0 .. nb - 1, nb = ceil(n / 16); wave w owns the block rows ib >= j with ib % 4 == w, at most 8, their
//      16 x 16 accumulators in registers from (b) to (e):
//      (a) K(ib, j) + noise I by the general evaluator (eval_program<D, 4, 0>) on the short kernel's lane map, which is the MFMA
//          accumulator layout — lane (i = l % 16, q = l / 16), register r <-> element (i, 4 r + q); rows / columns past n are
//          identity (cov_finalize).  The block goes to its own slot of the workspace and the same lanes load it back as the
//          accumulator: held in registers across the evaluator's code, eight accumulators spilled (13 / 48 VGPRs at D = 4 / 8);
//          2 KiB out and in per block beside the j blocks stage (b) reads for it;
//      (b) for k < j: acc(ib) -= L(ib, k) L(j, k)' on v_mfma_f64_16x16x4, both operands straight from the workspace in operand
//          layout (blk[64 s4 + l]: 512 contiguous bytes per wave and slice); L(j, k) is loaded once per wave and k, the wave's up to
//          eight chains are independent (long_update: one loop body per number of rows, the next step's operands prefetched);
//      (c) the wave that owns row j puts S(j, j) into LDS and factors it (factor16 on a one-block triangle: L(j, j) in place, its
//          inverse in Wl); barrier;
//      (d) panel L(ib, j) = S(ib, j) W' from the registers (lds_chol_steps' stage (b)) -> workspace, L(j, j) -> workspace;
//          alpha_j = W r_j with one refinement step against L(j, j) (lds_chol_steps' statements) and 2 log L_ii of the block's
//          rows, by 16 lanes of wave 3; barrier;
//      (e) r_ib -= L(ib, j) alpha_j from the registers, the four lane groups of a row in the order ((q0 + q1) + q2) + q3.
//      Two workgroup barriers per block column are all the ordering the workspace needs: every block is written and read by the
//      same workgroup on one CU, nothing crosses workgroups.  No look-ahead: while one wave factors the diagonal block the other
//      three wait; a second workgroup on the CU fills the gap (not measured against a look-ahead variant).
//   4. out_logpdf[p] = -(n log 2 pi + 2 sum log L_ii + alpha'alpha) / 2, both sums in a fixed order; on a bad pivot NaN and
//      out_info[p] = the first non-positive pivot, 1-based (each wave keeps the first it saw; the smallest is the first).
// k_long_series_logpdf<4, true> is the probe (agp_debug_long_series_factor, LongSeriesProbeArgs): stage 1 loads the caller's
// right-hand side, stage 2 is absent and stage 3 (a) writes the caller's block — in the evaluator's lane map, a diagonal block
// mirrored from the lower triangle, identity past n — into the block's slot; from the accumulator read-back on, (b) - (e) and stage 4
// are the statements above.  It also writes out the two partials and alpha; the packed blocks are the workspace.  A translation
// unit of its own (agp_kernels_long_series_probe.hip), so that the production instantiations compile as they did without it.
// 246 VGPRs, no AGPRs, 0 VGPRs spilled, scratch 0 bytes per lane, 73 SGPRs kept in VGPR lanes, 2 waves per SIMD (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950).
// k_long_series_predict<D> = k_long_series_logpdf<D, false, LongSeriesPredArgs> is the predictive twin (agp_predict_long_series_batch):
// per-point tables of LONG_PRED_SIG_STRIDE entries, factor16<true> also leaves W(j) = L(j, j)^-1 behind the triangle, and stage P
// (below, behind stage 4) forms the posterior at the series' own query times.  A unit of its own as well
// (agp_kernels_long_series_predict.hip, which records its registers, LDS and workspace).
// k_long_series_predict_logpdf<D> = k_long_series_logpdf<D, false, LongSeriesProbaArgs> is the held-out twin
// (agp_predict_logpdf_long_series_batch): the statements above on the JOINT points of the series — its ntr = n_s training points
// followed, without padding, by its mq query points, n = ntr + mq <= 512 — in long_series_lds(n, ..) and the value kernel's workspace.
// Every statement of its own is behind the trait JOINT (which a sampling twin would share, as PROBA and SAMPLE do in series_body):
// stage 1 reads the query times and the held-out values behind the series' own; stage 3 (a) adds noise to the diagonal of the rows
// below ntr and noise_pred from there on; stage 4 reduces over the rows [ntr, n) alone, a row in front of them contributing an exact
// 0.0 in its place of the fixed order — out_lp = -(mq log 2 pi + ld + ss) / 2 + mq log|slope|, the bits of the value kernel when
// ntr = 0 and the slope is 1 —; out_info is the first bad pivot on the joint index; behind stage 4's barrier the per-point terms
// (-(z_k^2 + log 2 pi) / 2 - log L_kk) + log|slope| of the rows k = ntr + j are written from avec and ldg, NaN in the whole block
// after a bad pivot.  No barrier is added to the block-column loop.  A unit of its own as well
// (agp_kernels_long_series_proba.hip, which records its registers, LDS and workspace).
// A particle's bits depend on its own series, program, parameters and noise only: the LDS map (long_series_lds, agp_args.hpp) is a
// function of the particle's own sizes, the workspace is the workgroup's own, no value crosses workgroups.
//
// LDS: Wl and the diagonal block 4 KiB, ts / r / alpha / log-diagonal 4 x 8 np B (16 KiB at 512), exponential table 1 KiB, the
// program, 4 KiB per ChangePoint node: 61 KiB beside 10 nodes, so two workgroups share a CU; one workgroup's 160 KiB hold 34 nodes
// beside a small program (the host refuses what does not fit).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), D = 4 and D = 8 alike: 255 VGPRs, no AGPRs, 0 VGPRs spilled,
// scratch 0 bytes per lane, 2 waves per SIMD (__launch_bounds__(256, 2)); 150 SGPRs are kept in VGPR lanes, as 93 to 114 are in the
// family's predictive kernels.
#pragma once
#include "agp_common.hpp"
#include "agp_args.hpp"
#include "agp_cov_kernel.hpp"
#include "agp_lds_chol.hpp"         // mfma, blk_idx, factor16, readlane_d

namespace agp {

constexpr int LONG_ROWS_PER_WAVE = LONG_SERIES_MAX_N / 16 / 4;      // block rows one wave owns at most
static_assert(LONG_ROWS_PER_WAVE * 64 == LONG_SERIES_MAX_N, "the cap is whole rounds of the four waves");
static_assert(LONG_SIG_STRIDE >= LONG_SERIES_MAX_N, "a per-point table holds the whole series");

// sigma_cp (src/GP.jl:481-483) of every ChangePoint node at time t -> entry `slot` of the node's table (series_sigma_cp's arithmetic)
template <int STRIDE = LONG_SIG_STRIDE>
__device__ __forceinline__ void long_sigma_cp(const ProgHdr& h, const int* ops, const double* prm, double* sig, int slot, double t) {
  int q = 0, c = 0;
  for (int ip = 0; ip < h.n_ops; ++ip) {
    const int o = ops[ip];
    if (o == OP_CP || o == OP_CP_SWAP) {
      const double loc = prm[q], sc = prm[q + 1];
      sig[c * STRIDE + slot] = 0.5 * (1.0 + tanh((loc - t) / sc));
      ++c;
    }
    q += prm_count(o);
  }
}

// Stage (b) of one wave with C block rows ib0, ib0 + 4, ..: acc(u) -= sum_{k < j} L(ib0 + 4 u, k) L(j, k)', j > 0.  The C chains are
// independent, interleaved slice by slice as in lds_chol_steps; every element is one chain over k in ascending order.  C <= 6: the
// operands of step k + 1 are on their way from the workspace while the MFMAs of step k run (the last step loads its own operands
// again).  With seven or eight rows a second operand set does not fit the 256 registers beside the accumulators (it spilled 10
// VGPRs); those chains are at most eight steps long.  Tried and dropped: a ring of 6 / 4 / 3 operand sets for waves with one to three
// rows (the late columns' long chains) measured the same — kernels 1.214 against 1.215 ms at 64 series x 442 points x 8 particles,
// 0.716 against 0.704 ms for one series — so the workspace's latency is not what a block column waits for: the evaluator (101
// blocks per wave at 442 points) and the wave-serial factor16 are.  Deeper rings spilled 29 to 59 VGPRs.
template <int C>
__device__ __forceinline__ void long_update(d4 (&acc)[LONG_ROWS_PER_WAVE], const double* ws, int j, int ib0, int l) {
  constexpr bool PREFETCH = C <= 6;
  const double* la = ws + blk_idx(j, 0) * 256 + l;      // row j's blocks are consecutive
  const double* lb[C];
#pragma unroll
  for (int u = 0; u < C; ++u) lb[u] = ws + blk_idx(ib0 + 4 * u, 0) * 256 + l;
  double fa[4], fb[C][4];
  if constexpr (PREFETCH) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      fa[s4] = la[64 * s4];
#pragma unroll
      for (int u = 0; u < C; ++u) fb[u][s4] = lb[u][64 * s4];
    }
  }
  for (int k = 0; k < j; ++k) {
    if constexpr (PREFETCH) {
      const int kn = (k + 1 < j ? k + 1 : k) * 256;
      double na[4], nb[C][4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        na[s4] = la[kn + 64 * s4];
#pragma unroll
        for (int u = 0; u < C; ++u) nb[u][s4] = lb[u][kn + 64 * s4];
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int u = 0; u < C; ++u) acc[u] = mfma(-fa[s4], fb[u][s4], acc[u]);
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        fa[s4] = na[s4];
#pragma unroll
        for (int u = 0; u < C; ++u) fb[u][s4] = nb[u][s4];
      }
    } else {
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        fa[s4] = la[k * 256 + 64 * s4];
#pragma unroll
        for (int u = 0; u < C; ++u) fb[u][s4] = lb[u][k * 256 + 64 * s4];
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int u = 0; u < C; ++u) acc[u] = mfma(-fa[s4], fb[u][s4], acc[u]);
    }
  }
}

// One body for the value kernel, its probe, the predictive and the held-out twin, selected by the argument type (as series_body is
// for the short family): every statement of a twin's own is behind PRED or JOINT.  The body is the kernel itself, not a function the three kernels call:
// inlined from a function its early returns become branches to a common end, and the value and the probe instantiation then
// allocate their registers differently (tried: by reference, by value, the LDS symbol declared inside).  As it stands their
// instructions are those of the kernel without the twin; their symbols carry the argument type.
template <int D, bool PROBE = false, class ArgsT = std::conditional_t<PROBE, LongSeriesProbeArgs, LongSeriesArgs>>
__global__ __launch_bounds__(256, 2) void k_long_series_logpdf(ArgsT a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr bool PRED = std::is_same_v<ArgsT, LongSeriesPredArgs>;
  constexpr bool PROBA = std::is_same_v<ArgsT, LongSeriesProbaArgs>;      // the held-out twin: n below is the JOINT length
  constexpr bool JOINT = PROBA;      // (the branches of the joint points: a sampling twin would share them, as in series_body)
  constexpr int STRIDE = PRED ? LONG_PRED_SIG_STRIDE : LONG_SIG_STRIDE;      // entries of one per-point table
  constexpr int E = 4, U = LONG_ROWS_PER_WAVE;
  const int tid = threadIdx.x, l = tid & 63, l15 = l & 15, lq = l >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // (on the scalar unit: which block rows a wave owns is wave-uniform control flow)
  int p, n;
  [[maybe_unused]] long long o0 = 0;
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
      n = (mq <= 0 || mq > LONG_SERIES_MAX_N) ? 0 : n + (int)mq;      // (nothing held out: never launched, like an empty series)
    }
  }
  if (n <= 0 || n > LONG_SERIES_MAX_N) {      // (the host answers empty series itself and refuses longer ones: never launched)
    if (tid == 0) { a.out_lp[p] = 0.0; a.out_info[p] = 0; }
    return;
  }
  const ProgHdr h = [&]() -> ProgHdr { if constexpr (PROBE) return ProgHdr{}; else return a.hdr[p]; }();
  const LongSeriesLds m = PRED ? long_series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp) : long_series_lds(n, h.n_ops, h.n_prm, h.n_cp);
  const int nb = m.nb, np = m.np;
  double* Wl = smem;
  double* dblk = smem + m.o_dblk;
  [[maybe_unused]] double* tpt = smem + m.o_tpt;      // (tpt, etab, prm, ops, sig: unused by the probe)
  double* rvec = smem + m.o_rvec;
  double* avec = smem + m.o_avec;
  double* ldg = smem + m.o_ldg;
  [[maybe_unused]] double* etab = smem + m.o_etab;
  [[maybe_unused]] double* prm = smem + m.o_prm;
  [[maybe_unused]] int* ops = reinterpret_cast<int*>(smem + m.o_ops);
  [[maybe_unused]] double* sig = smem + m.o_sig;
  double* ws = a.ws + (long long)blockIdx.x * a.ws_stride;
  [[maybe_unused]] double* wsW = nullptr;      // PRED: the nb inverses W(j) behind the triangle and the round's scratch rows
  if constexpr (PRED) wsW = ws + long_series_ws_blocks(nb + 4 * LONG_PRED_C) * 256;

  // ---- 1. inputs (the probe: the caller's right-hand side) ----
  if constexpr (PROBE) {
    for (int i = tid; i < np; i += 256) {
      rvec[i] = (i < n && a.y != nullptr) ? a.y[(long long)p * n + i] : 0.0;
      avec[i] = 0.0;
    }
    __syncthreads();
  } else {
    if constexpr (JOINT) {
      // the joint points: the series' times, then — directly behind them, no padding between — its query times; xs, then the held-out values
      for (int i = tid; i < np; i += 256) {
        const int k = i < n ? i : n - 1;
        tpt[i] = k < ntr ? a.ts[o0 + k] : a.ts_pred[q0 + (k - ntr)];
        rvec[i] = i < ntr ? a.xs[o0 + i] : i < n ? a.y_pred[q0 + (i - ntr)] : 0.0;
        avec[i] = 0.0;
      }
    } else {
      for (int i = tid; i < np; i += 256) {
        tpt[i] = a.ts[o0 + (i < n ? i : n - 1)];      // (padding points: a finite time; their entries are overwritten with identity)
        rvec[i] = i < n ? a.xs[o0 + i] : 0.0;
        avec[i] = 0.0;
      }
    }
    if (AGP_EXP_TABLE && tid < AGP_EXP_TAB_N) etab[tid] = fm::c_exp_tab[tid];
    for (int i = tid; i < h.n_prm + 2; i += 256) prm[i] = a.prm[h.prm_off + i];      // (the parameter buffer carries two doubles of tail padding)
    for (int i = tid; i < h.n_ops; i += 256) ops[i] = (int)a.ops[h.op_off + i];
    __syncthreads();

    // ---- 2. per-point tables ----
    if (h.n_cp > 0) {
      for (int i = tid; i < np; i += 256) long_sigma_cp<STRIDE>(h, ops, prm, sig, i, tpt[i]);
      __syncthreads();
    }
  }

  // ---- 3. block columns ----
  [[maybe_unused]] const double noise = [&]() { if constexpr (PROBE) return 0.0; else return a.noise[p]; }();
  [[maybe_unused]] double noise_q = 0.0;      // JOINT: the diagonal addend of the query rows
  if constexpr (JOINT) noise_q = a.noise_pred[p];
  int bad = 0;           // first non-positive pivot this wave has seen (1-based index in the series), 0 = none
  for (int j = 0; j < nb; ++j) {
    const int ib0 = j + ((w - j) & 3);      // the wave's first block row at or below j
    // (a) K(ib, j) + noise I -> the block's own slot of the workspace (the lanes that wrote an entry read it back below)
    // (the probe: the caller's block instead, a diagonal block mirrored from the lower triangle, identity past n as cov_finalize makes it)
    for (int ib = ib0; ib < nb; ib += 4) {
      double* kb = ws + blk_idx(ib, j) * 256;
      if constexpr (PROBE) {
        const double* Kp = a.K + (long long)p * n * n;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int ri = ib * 16 + l15, ci = j * 16 + lq + 4 * e;
          const int hi = ri > ci ? ri : ci, lo = ri > ci ? ci : ri;
          kb[64 * e + l] = hi < n ? Kp[(long long)hi * n + lo] : (ri == ci ? 1.0 : 0.0);
        }
      } else {
        double tr[E], tc[E], out[E], lt[E];
        int ri[E], ci[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          ri[e] = ib * 16 + l15;
          ci[e] = j * 16 + lq + 4 * e;
          tr[e] = tpt[ri[e]];
          tc[e] = tpt[ci[e]];
          lt[e] = 0.0;
        }
        eval_program<D, E, 0, false, STRIDE>(h, ops, prm, sig, tr, tc, ri, ci, lt, out, etab);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if constexpr (JOINT) kb[64 * e + l] = cov_finalize(out[e], ri[e], ci[e], n, np, 0, ri[e] < ntr ? noise : noise_q);
          else kb[64 * e + l] = cov_finalize(out[e], ri[e], ci[e], n, np, 0, noise);
        }
      }
    }
    d4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[u] = d4{0.0, 0.0, 0.0, 0.0};
      if (ib0 + 4 * u < nb) {
        const double* kb = ws + blk_idx(ib0 + 4 * u, j) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][r] = kb[64 * r + l];
      }
    }
    // (b) acc(ib) -= sum_{k < j} L(ib, k) L(j, k)': the wave's rows are u = 0 .. cnt - 1; one straight-line loop body per count
    if (j > 0 && ib0 < nb) {
      const int cnt = (nb - 1 - ib0) / 4 + 1;
      switch (cnt) {
        case 1: long_update<1>(acc, ws, j, ib0, l); break;
        case 2: long_update<2>(acc, ws, j, ib0, l); break;
        case 3: long_update<3>(acc, ws, j, ib0, l); break;
        case 4: long_update<4>(acc, ws, j, ib0, l); break;
        case 5: long_update<5>(acc, ws, j, ib0, l); break;
        case 6: long_update<6>(acc, ws, j, ib0, l); break;
        case 7: long_update<7>(acc, ws, j, ib0, l); break;
        default: long_update<8>(acc, ws, j, ib0, l); break;
      }
    }
    // (c) the diagonal block: the wave that owns row j holds it in acc[0]
    if (w == (j & 3)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dblk[64 * r + l] = acc[0][r];
      if constexpr (PRED) factor16<true>(dblk, Wl, wsW + j * 256, 0, j * 16, bad, l);      // (W(j) also to its slot behind the triangle)
      else factor16<false>(dblk, Wl, nullptr, 0, j * 16, bad, l);
    }
    __syncthreads();
    // (d) panel L(ib, j) = S(ib, j) W' -> workspace; alpha_j, 2 log L_ii
    {
      double fw[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) fw[s4] = Wl[64 * s4 + l];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ib = ib0 + 4 * u;
        if (ib > j && ib < nb) {
          d4 x = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) x = mfma(fw[s4], acc[u][s4], x);
          acc[u] = x;
          double* lb = ws + blk_idx(ib, j) * 256;
#pragma unroll
          for (int r = 0; r < 4; ++r) lb[64 * r + l] = x[r];
        }
      }
      if (w == (j & 3)) {
        double* lb = ws + blk_idx(j, j) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) lb[64 * r + l] = dblk[64 * r + l];
      }
    }
    if (w == 3 && l < 16) {
      // alpha_j = W r_j, then ONE step of refinement against the block itself (lds_chol_steps' statements)
      double wr[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) wr[q] = Wl[q * 16 + l];
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        t0 = fma(wr[q], rvec[j * 16 + q], t0);
        t1 = fma(wr[q + 1], rvec[j * 16 + q + 1], t1);
      }
      const double a0 = t0 + t1;
      double r0 = rvec[j * 16 + l], r1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        r0 = fma(-dblk[q * 16 + l], readlane_d(a0, q), r0);
        r1 = fma(-dblk[(q + 1) * 16 + l], readlane_d(a0, q + 1), r1);
      }
      const double rho = r0 + r1;
      double c0 = 0.0, c1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        c0 = fma(wr[q], readlane_d(rho, q), c0);
        c1 = fma(wr[q + 1], readlane_d(rho, q + 1), c1);
      }
      avec[j * 16 + l] = a0 + (c0 + c1);
      ldg[j * 16 + l] = 2.0 * log(dblk[17 * l]);      // (padding rows: log 1)
    }
    __syncthreads();
    // (e) r_ib -= L(ib, j) alpha_j, from the registers
    {
      double al[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) al[r] = avec[j * 16 + 4 * r + lq];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ib = ib0 + 4 * u;
        if (ib > j && ib < nb) {
          double t = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) t = fma(acc[u][r], al[r], t);
          const double s = ((__shfl(t, l15) + __shfl(t, l15 + 16)) + __shfl(t, l15 + 32)) + __shfl(t, l15 + 48);
          if (l < 16) rvec[ib * 16 + l] -= s;
        }
      }
    }
  }

  // ---- 4. the value: 2 sum log L_ii and alpha'alpha, reduced in a fixed order; the first bad pivot of the four waves ----
  if (l == 0) dblk[w] = (double)bad;      // (the last diagonal block has been consumed)
  // (JOINT: both sums over the query rows [ntr, n) alone — the conditional density of the held-out values; a row in front of them
  // contributes an exact 0.0 in its place of the same fixed order, so with ntr = 0 the sums are the value kernel's)
  if constexpr (JOINT) Wl[tid] = (tid >= ntr && tid < np ? ldg[tid] : 0.0) + (tid + 256 >= ntr && tid + 256 < np ? ldg[tid + 256] : 0.0);
  else Wl[tid] = (tid < np ? ldg[tid] : 0.0) + (tid + 256 < np ? ldg[tid + 256] : 0.0);      // (the last inverse block likewise)
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
      int first = 0;
      for (int k = 0; k < 4; ++k) {
        const int b = (int)dblk[k];
        if (b != 0 && (first == 0 || b < first)) first = b;
      }
      double lp;
      if constexpr (JOINT) {
        // m log 2 pi, and the Jacobian of the series' own transform: m log|slope|.  The first product and sum are written as the
        // fused operation the value kernel's statement below compiles to, so that with ntr = 0 and slope 1 the bits are that
        // kernel's whatever the compiler makes of the longer expression (tests/test_gpu_long_series_proba.py compares them)
        const double mq = (double)(n - ntr);
        lp = -0.5 * (fma(mq, 1.8378770664093454835606594728112, ld) + ss) + mq * log(fabs(a.y_slope[a.series[p]]));
      } else {
        lp = -0.5 * ((double)n * 1.8378770664093454835606594728112 + ld + ss);
      }
      a.out_lp[p] = first != 0 ? __builtin_nan("") : lp;
      a.out_info[p] = first;
      if constexpr (PROBE) { a.out_part[2 * p] = ld; a.out_part[2 * p + 1] = ss; }
    }
  }
  if constexpr (PROBE)      // alpha as stage 3 left it (the packed blocks are in the workspace)
    for (int i = tid; i < np; i += 256) a.out_alpha[(long long)p * np + i] = avec[i];

  if constexpr (PROBA) {
    // ---- the per-point terms: log N(y_j | training data, y_0 .. y_{j-1}) from row ntr + j of the joint factor (chain rule).  Behind
    // stage 4's barrier alpha (avec) and the log-diagonal (ldg = 2 log L_kk) are read-only and the four first-bad-pivot words in
    // dblk are written: no further barrier ----
    if (a.out_terms != nullptr) {
      const bool failed = dblk[0] != 0.0 || dblk[1] != 0.0 || dblk[2] != 0.0 || dblk[3] != 0.0;      // NaN in the particle's whole block
      const double lsl = log(fabs(a.y_slope[a.series[p]]));
      double* ot = a.out_terms + a.out_off[p];
      for (int k = ntr + tid; k < n; k += 256) {
        const double z = avec[k];
        const double t = (-0.5 * fma(z, z, 1.8378770664093454835606594728112) - 0.5 * ldg[k]) + lsl;
        ot[k - ntr] = failed ? __builtin_nan("") : t;
      }
    }
  }

  if constexpr (PRED) {
    // ---- P. the posterior at the series' own query times: mean = VT alpha, var = (k(t*, t*) - rowsums(VT^2)) + noise_pred, VT = K21 L^-T.
    // Behind stage 4's barrier the factor, the inverses W(j), alpha (avec; padding: 0), tpt, the program and its tables are
    // read-only and the four first-bad-pivot words in dblk are written: no further workgroup barrier.  Query block qb (16 times)
    // belongs to wave qb % 4; a wave runs its blocks in rounds of up to LONG_PRED_C chains, chain u in scratch row nb + w + 4 u:
    //   sigma_cp of the chain's 16 times -> entries LONG_PRED_QSLOT + 16 (LONG_PRED_C w + u) .. of every per-point table (wave-local);
    //   for j = 0 .. nb - 1: K21(q, j) by the evaluator on stage 3's lane map (columns past n: 0) -> block j of the scratch row, and
    //     back as the accumulator; S(q, j) = K21(q, j) - sum_{k < j} VT(q, k) L(j, k)' by long_update, the chains sharing L(j, k);
    //     VT(q, j) = S(q, j) W(j)' -> block j of the scratch row (accumulator and operand layout coincide, blk[64 r + l]: a lane
    //     reads back only what it stored itself); the lane's share of mean and of rowsums(VT^2), ascending in (j, r);
    //   "block" nb: k(t*, t*) through the same call of the evaluator, row and column both the query, by way of block nb of the row;
    //   the four lane groups of a row in the order ((q0 + q1) + q2) + q3.
    // Rows past mq evaluate the last query time again and are not written; a chain's arithmetic is the same whichever round and
    // whichever count of chains it runs in (long_update's chains are independent).
    constexpr int C = LONG_PRED_C;
    const int sidx = a.series[p];
    const long long q0 = a.q_off[sidx];
    const int mq = (int)(a.q_off[sidx + 1] - q0);
    if (mq <= 0) return;
    double* om = a.out_mean + a.out_off[p];
    double* ov = a.out_var + a.out_off[p];
    if (dblk[0] != 0.0 || dblk[1] != 0.0 || dblk[2] != 0.0 || dblk[3] != 0.0) {      // a bad pivot: NaN in the particle's whole block
      for (int q = tid; q < mq; q += 256) { om[q] = __builtin_nan(""); ov[q] = __builtin_nan(""); }
      return;
    }
    const double* tq = a.ts_pred + q0;
    const double noise_pred = a.noise_pred[p];
    const int row0 = nb + w;      // the wave's first scratch row
    for (int qb0 = w; qb0 * 16 < mq; qb0 += 4 * C) {
      const int left = (mq - qb0 * 16 + 63) / 64;      // the wave's query blocks from qb0 on
      const int cnt = left < C ? left : C;
      double tqu[C], ms[C], ss[C], kd[C];
#pragma unroll
      for (int u = 0; u < C; ++u) {
        const int qi = (qb0 + 4 * u) * 16 + l15;
        tqu[u] = tq[qi < mq ? qi : mq - 1];
        ms[u] = 0.0; ss[u] = 0.0; kd[u] = 0.0;
        if (h.n_cp > 0 && u < cnt && l < 16) long_sigma_cp<STRIDE>(h, ops, prm, sig, LONG_PRED_QSLOT + 16 * (C * w + u) + l15, tqu[u]);
      }
      __builtin_amdgcn_wave_barrier();      // (LDS operations of one wave complete in order: its own lanes' entries)
      for (int j = 0; j <= nb; ++j) {
        const bool self = j == nb;
        // K21(q_u, j) (self: k(t*, t*), every register alike) -> block j of scratch row u
        for (int u = 0; u < cnt; ++u) {
          const int slot = LONG_PRED_QSLOT + 16 * (C * w + u) + l15;
          double tr[E], tc[E], out[E], lt[E];
          int ri[E], ci[E];
          double tu = tqu[0];
#pragma unroll
          for (int v = 1; v < C; ++v) tu = u == v ? tqu[v] : tu;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            ri[e] = slot;
            ci[e] = self ? slot : j * 16 + lq + 4 * e;
            tr[e] = tu;
            tc[e] = self ? tu : tpt[ci[e]];
            lt[e] = 0.0;
          }
          eval_program<D, E, 0, false, STRIDE>(h, ops, prm, sig, tr, tc, ri, ci, lt, out, etab);
          double* kb = ws + blk_idx(row0 + 4 * u, j) * 256;
#pragma unroll
          for (int e = 0; e < E; ++e) kb[64 * e + l] = (self || ci[e] < n) ? out[e] : 0.0;
        }
        if (self) {
#pragma unroll
          for (int u = 0; u < C; ++u)
            if (u < cnt) kd[u] = ws[blk_idx(row0 + 4 * u, j) * 256 + l];
          break;
        }
        d4 acc[U];
#pragma unroll
        for (int u = 0; u < C; ++u) {
          acc[u] = d4{0.0, 0.0, 0.0, 0.0};
          if (u < cnt) {
            const double* kb = ws + blk_idx(row0 + 4 * u, j) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[u][r] = kb[64 * r + l];
          }
        }
        if (j > 0) {
          static_assert(C == 2, "one loop body per number of chains");
          if (cnt == 1) long_update<1>(acc, ws, j, row0, l);
          else long_update<2>(acc, ws, j, row0, l);
        }
        double fw[4], al[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) { fw[s4] = wsW[j * 256 + 64 * s4 + l]; al[s4] = avec[j * 16 + 4 * s4 + lq]; }
#pragma unroll
        for (int u = 0; u < C; ++u)
          if (u < cnt) {
            d4 x = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) x = mfma(fw[s4], acc[u][s4], x);
            double* vb = ws + blk_idx(row0 + 4 * u, j) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              vb[64 * r + l] = x[r];
              ms[u] = fma(x[r], al[r], ms[u]);
              ss[u] = fma(x[r], x[r], ss[u]);
            }
          }
      }
#pragma unroll
      for (int u = 0; u < C; ++u)
        if (u < cnt) {
          const double mean = ((__shfl(ms[u], l15) + __shfl(ms[u], l15 + 16)) + __shfl(ms[u], l15 + 32)) + __shfl(ms[u], l15 + 48);
          const double sq = ((__shfl(ss[u], l15) + __shfl(ss[u], l15 + 16)) + __shfl(ss[u], l15 + 32)) + __shfl(ss[u], l15 + 48);
          const int qi = (qb0 + 4 * u) * 16 + l15;
          if (l < 16 && qi < mq) {
            om[qi] = mean;
            ov[qi] = (kd[u] - sq) + noise_pred;
          }
        }
    }
  }
}

// The predictive twin (agp_predict_long_series_batch; agp_kernels_long_series_predict.hip has its figures)
template <int D> constexpr auto k_long_series_predict = &k_long_series_logpdf<D, false, LongSeriesPredArgs>;
// The held-out twin (agp_predict_logpdf_long_series_batch; agp_kernels_long_series_proba.hip has its figures)
template <int D> constexpr auto k_long_series_predict_logpdf = &k_long_series_logpdf<D, false, LongSeriesProbaArgs>;

}  // namespace agp
