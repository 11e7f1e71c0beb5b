// The 16x16-blocked right-looking fp64 Cholesky that runs entirely in LDS with the forward solve carried along — ONE copy behind
// the diagonal tile of the tiled sweeps (factor_diag_tile, agp_chol_kernel.hpp: 8 block rows, compile time) and the short-series
// kernels (series_body, agp_series_kernel.hpp: ceil(n / 16) <= 11 block rows, run time).
//
// Layout both callers stage: the lower 16 x 16 blocks of the matrix packed by rows, block (rb, cb) column-major at
// sm + blk_idx(rb, cb) * 256 (a diagonal block holds both triangles; rows / columns past the data are identity); Wl = 256 doubles for
// the inverse of the current diagonal block; rvec = the right-hand side, avec = the solution, one double per row.  256 threads.
#pragma once
#include "agp_common.hpp"

namespace agp {

__device__ __forceinline__ double readlane_d(double v, int lane) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, lane);
  hi = __builtin_amdgcn_readlane(hi, lane);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int blk_idx(int rb, int cb) { return rb * (rb + 1) / 2 + cb; }

__device__ __forceinline__ void sqrt_rsqrt(double d, double& sq, double& ri) {
  // v_rsq_f64 is good to ~2^-23; ONE third-order step y (1 + e/2 + 3 e^2 / 8), e = 1 - d y^2, leaves e^3 ~ 2^-69: four
  // dependent operations behind the estimate instead of the six of two coupled second-order steps (this is the tile's serial chain)
  const double y = __builtin_amdgcn_rsq(d);
  const double t = d * y;
  const double e = fma(-t, y, 1.0);
  const double pq = fma(e, 0.375, 0.5), ye = y * e;
  ri = fma(ye, pq, y);
  // sqrt(d) = d ri, corrected once with the residual (off the chain: only the stored diagonal entry reads it)
  const double g = d * ri;
  sq = fma(fma(-g, g, d), 0.5 * ri, g);
}

// the probe of a caller that has none
struct LdsCholNoProbe { __device__ __forceinline__ void operator()(int) const { } };

// 16x16 Cholesky of block (jb,jb) + its inverse, run by ONE wave (l = lane), 4 columns at a time on the matrix pipe.
// The block sits in the wave's registers as Y[r], lane (i = l%16, q = l/16) <-> S[i][4r + q] (= blk[64 r + l]): register
// r' is at once the A- and the B-operand fragment of columns 4r' .. 4r'+3.  Sub-step r':
//   1. the 4 x 4 diagonal sub-block goes to the scalar unit (10 v_readlane pairs); every lane factors it and inverts the
//      factor redundantly (W4: the only serial chain — four v_rsq_f64 + Goldschmidt steps per sub-step);
//   2. columns: L[:, 4r' ..] = S[:, 4r' ..] W4^T is ONE MFMA, (W4 padded to 16 x 4) x Y[r'], whose result register 0 lands in
//      the operand layout again (lane (i, q) <-> L[i][4r' + q]);
//   3. trailing columns: Y -= L[c >= 4r'+4, 4r' ..] L[:, 4r' ..]^T is ONE more MFMA (A rows of finished columns zeroed).
// An identity block rides along through 2. and 3.: what happens to the rows of a block below the diagonal, X = S L^-T, turns
// I into L^-T — its transposed storage is L^-1, the inverse the panel solves need.  About 120 vector instructions + 4 MFMAs
// per sub-step instead of the ~250 of a column-by-column elimination on v_readlane broadcasts (r03: 2.4 us per block, the
// longest phase of the tile's dependency chain).
// bad: the first non-positive pivot so far, 1-based, counted from pivot_base (0 = none).  The inverse goes to Wl and, with WHBM, to
// the 256 doubles at Wg + jb * 256 in HBM as well.
// (Not __forceinline__: inlined before the optimiser has seen it on its own — as a lambda never is — the pivot tests compile to mask
// arithmetic instead of scalar selects and the tile kernels spill more; profiles/lds_chol_fold_isa.txt.)
template <bool WHBM>
__device__ void factor16(double* sm, double* Wl, double* Wg, int jb, int pivot_base, int& bad, int l) {
  const int l15 = l & 15, lq = l >> 4;
  double* blk = sm + blk_idx(jb, jb) * 256;
  d4 Y0, Yw;
#pragma unroll
  for (int r = 0; r < 4; ++r) { Y0[r] = blk[64 * r + l]; Yw[r] = (l15 == 4 * r + lq) ? 1.0 : 0.0; }
  const int dlt = l15 - lq;
#pragma unroll
  for (int rp = 0; rp < 4; ++rp) {
    const int c0 = 4 * rp;
    // S[c0+a][c0+b], a >= b: register rp of lane 16 b + c0 + a
    const double d00 = readlane_d(Y0[rp], c0), d10 = readlane_d(Y0[rp], c0 + 1), d20 = readlane_d(Y0[rp], c0 + 2),
                 d30 = readlane_d(Y0[rp], c0 + 3), d11 = readlane_d(Y0[rp], 16 + c0 + 1), d21 = readlane_d(Y0[rp], 16 + c0 + 2),
                 d31 = readlane_d(Y0[rp], 16 + c0 + 3), d22 = readlane_d(Y0[rp], 32 + c0 + 2), d32 = readlane_d(Y0[rp], 32 + c0 + 3),
                 d33 = readlane_d(Y0[rp], 48 + c0 + 3);
    const int g0 = pivot_base + jb * 16 + c0;       // index of the sub-block's first pivot
    double l00, r0, l11, r1, l22, r2, l33, r3;
    if (!(d00 > 0.0) && bad == 0) bad = g0 + 1;
    sqrt_rsqrt(d00, l00, r0);
    const double l10 = d10 * r0, l20 = d20 * r0, l30 = d30 * r0;
    const double e11 = fma(-l10, l10, d11);
    if (!(e11 > 0.0) && bad == 0) bad = g0 + 2;
    sqrt_rsqrt(e11, l11, r1);
    const double l21 = fma(-l20, l10, d21) * r1, l31 = fma(-l30, l10, d31) * r1;
    const double e22 = fma(-l21, l21, fma(-l20, l20, d22));
    if (!(e22 > 0.0) && bad == 0) bad = g0 + 3;
    sqrt_rsqrt(e22, l22, r2);
    const double l32 = fma(-l31, l21, fma(-l30, l20, d32)) * r2;
    const double e33 = fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, d33)));
    if (!(e33 > 0.0) && bad == 0) bad = g0 + 4;
    sqrt_rsqrt(e33, l33, r3);
    // W4 = L4^-1 (lower).  Row 3 carries the factor 1/l33 of the LAST pivot: the lanes' values are selected without it while
    // that pivot's reciprocal root is still on its way, and multiplied afterwards (two operations behind r3 instead of six)
    const double w10 = -(l10 * r0) * r1, w21 = -(l21 * r1) * r2;
    const double w20 = -fma(l21, w10, l20 * r0) * r2;
    const double u32 = -(l32 * r2), u31 = -fma(l32, w21, l31 * r1), u30 = -fma(l32, w20, fma(l31, w10, l30 * r0));
    // A operand of the column step: lane 16 k + i <-> W4[i][k]
    double aW = 0.0;
    aW = (l == 0) ? r0 : aW;   aW = (l == 1) ? w10 : aW;  aW = (l == 17) ? r1 : aW;
    aW = (l == 2) ? w20 : aW;  aW = (l == 18) ? w21 : aW; aW = (l == 34) ? r2 : aW;
    double u3 = 1.0;
    u3 = (l == 3) ? u30 : u3;  u3 = (l == 19) ? u31 : u3; u3 = (l == 35) ? u32 : u3;
    aW = (l15 == 3) ? u3 * r3 : aW;
    const d4 z4 = d4{0.0, 0.0, 0.0, 0.0};
    const d4 T0 = mfma(aW, Y0[rp], z4);      // T0[0], lane (i, q): L[i][c0 + q] (rows i < c0: upper-triangle debris)
    const d4 Tw = mfma(aW, Yw[rp], z4);
    double nl = (dlt >= c0) ? T0[0] : 0.0;      // the finished columns: zero above the diagonal
    if (rp < 3) {
      const double nA = (l15 >= c0 + 4) ? -nl : 0.0;
      Y0 = mfma(nA, nl, Y0);
      Yw = mfma(nA, Tw[0], Yw);
    }
    // ... and the diagonal itself from the scalar factorisation
    nl = (l == c0) ? l00 : nl; nl = (l == 17 + c0) ? l11 : nl; nl = (l == 34 + c0) ? l22 : nl; nl = (l == 51 + c0) ? l33 : nl;
    Y0[rp] = nl;
    Yw[rp] = Tw[0];
  }
  double* Wgj = nullptr;
  if constexpr (WHBM) Wgj = Wg + jb * 256;      // (formed once: inside the store loop the tile kernels spill more)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    blk[64 * r + l] = Y0[r];
    // Yw[r], lane (i, q) <-> (L^-1)[4r + q][i]; W is kept column-major like every 16 x 16 block
    Wl[l15 * 16 + 4 * r + lq] = Yw[r];
    if constexpr (WHBM) Wgj[l15 * 16 + 4 * r + lq] = Yw[r];
  }
}

// The block steps jb = 0 .. nsteps - 1 over a triangle of nb block rows (NBR > 0: nb = NBR at compile time and nb_rt is ignored;
// NBR = 0: nb = nb_rt), all 256 threads, barriers inside; on entry the blocks and rvec are staged and a barrier has passed.  Per step:
// panel L(ib,jb) = S(ib,jb) W^T, alpha_jb (W r_jb + one refinement step) -> avec, trailing updates, r_ib -= L(ib,jb) alpha_jb by
// thread rbase + (row) for the rows below the step and below rrows, and the next diagonal block factored by wave 0 beside the
// trailing updates.  nsteps < nb: the remaining block rows are identity padding whose steps the caller writes down itself.
// probe(i), i = 2 .. 8: the phase stamps of tools/native/diag_bench.hip (nothing unless AGP_DIAG_PROBE is defined there).
template <int NBR, bool WHBM = false, class Probe = LdsCholNoProbe>
__device__ __forceinline__ void lds_chol_steps(double* sm, double* Wl, double* rvec, double* avec, int nb_rt, int nsteps, int rbase,
                                               int rrows, int pivot_base, int& bad, int tid, double* Wg = nullptr,
                                               const Probe& probe = Probe{}) {
  const int nb = NBR > 0 ? NBR : nb_rt;
  const int l = tid & 63, w = tid >> 6;
  // Look-ahead inside the triangle: while waves 1-3 apply block column jb to the trailing blocks, wave 0 applies it to the
  // NEXT diagonal block only and factors that block at once — the wave-serial 16x16 step (the longest phase of an
  // iteration) runs beside the MFMA updates instead of in front of them.
  probe(2);
  if (w == 0) factor16<WHBM>(sm, Wl, Wg, 0, pivot_base, bad, l);
  probe(3);
  __syncthreads();
  probe(4);
  for (int jb = 0; jb < nsteps; ++jb) {
    // ---- (b) panel: L(ib,jb) = S(ib,jb) W^T for ib > jb (MFMA); alpha_jb = W r_jb ----
    // (two blocks per wave and pass, so one pass covers the eight block rows of a tile; their four-MFMA chains are interleaved —
    // one after the other each MFMA waits for its predecessor's result)
    for (int ib0 = jb + 1 + w; ib0 < nb; ib0 += 8) {
      const int ib1 = ib0 + 4;
      double* blk0 = sm + blk_idx(ib0, jb) * 256;
      double* blk1 = sm + blk_idx(ib1 < nb ? ib1 : ib0, jb) * 256;
      double fw[4], fs0[4], fs1[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) { fw[s4] = Wl[64 * s4 + l]; fs0[s4] = blk0[64 * s4 + l]; fs1[s4] = blk1[64 * s4 + l]; }
      d4 x0 = d4{0.0, 0.0, 0.0, 0.0}, x1 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) { x0 = mfma(fw[s4], fs0[s4], x0); x1 = mfma(fw[s4], fs1[s4], x1); }
#pragma unroll
      for (int r = 0; r < 4; ++r) blk0[64 * r + l] = x0[r];
      if (ib1 < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) blk1[64 * r + l] = x1[r];
      }
    }
    if (w == 3 && l < 16) {
      // alpha_jb = W r_jb, then ONE step of refinement against the block itself: rho = r_jb - L(jb,jb) alpha, alpha += W rho.
      // W r alone leaves |L alpha - r| at the roundings of W AND of the product (three roundings against a division's one at a
      // 1 x 1 block: 1.9 gamma_1, tests/test_gpu_factor_probe.py); the corrected alpha has substitution's componentwise residual.
      // (lanes 0 .. 15 of this wave hold the block's rows; values travel between them through v_readlane)
      const double* Lb = sm + blk_idx(jb, jb) * 256;
      double wr[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) wr[q] = Wl[q * 16 + l];
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        t0 = fma(wr[q], rvec[jb * 16 + q], t0);
        t1 = fma(wr[q + 1], rvec[jb * 16 + q + 1], t1);
      }
      const double a0 = t0 + t1;
      double r0 = rvec[jb * 16 + l], r1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        r0 = fma(-Lb[q * 16 + l], readlane_d(a0, q), r0);
        r1 = fma(-Lb[(q + 1) * 16 + l], readlane_d(a0, q + 1), r1);
      }
      const double rho = r0 + r1;
      double c0 = 0.0, c1 = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        c0 = fma(wr[q], readlane_d(rho, q), c0);
        c1 = fma(wr[q + 1], readlane_d(rho, q + 1), c1);
      }
      avec[jb * 16 + l] = a0 + (c0 + c1);
    }
    __syncthreads();
    if (jb == 0) probe(5);

    // ---- (c) trailing blocks (ib,cb), jb < cb <= ib: S(ib,cb) -= L(ib,jb) L(cb,jb)^T;
    //      r_ib -= L(ib,jb) alpha_jb ----
    {
      const int nrem = nb - 1 - jb;              // block rows below jb
      const int npair = nrem * (nrem + 1) / 2;
      // pair 0 is the next diagonal block (jb+1, jb+1): wave 0 takes it (and then factors it); waves 1-3 share the rest, three
      // blocks per pass with their MFMA chains interleaved (pairs e = w, w + 3, ... in row-major order of the trailing triangle)
      if (w == 0) {
        if (npair > 0) {
          double* blk = sm + blk_idx(jb + 1, jb + 1) * 256;
          const double* la = sm + blk_idx(jb + 1, jb) * 256;
          d4 x;
          double f[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) { x[r] = blk[64 * r + l]; f[r] = la[64 * r + l]; }
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) x = mfma(-f[s4], f[s4], x);
#pragma unroll
          for (int r = 0; r < 4; ++r) blk[64 * r + l] = x[r];
        }
      } else {
        // position of pair e in the triangle: row ii (0-based below jb+1), column cc <= ii
        int e = w, ii = 1, cc = w - 1;                     // e = 1, 2, 3 -> (1,0), (1,1), (2,0)
        if (cc > ii) { cc -= ii + 1; ++ii; }
        auto advance = [&](int& e_, int& ii_, int& cc_) {  // three pairs on
          e_ += 3; cc_ += 3;
          while (cc_ > ii_) { cc_ -= ii_ + 1; ++ii_; }
        };
        while (e < npair) {
          int eb[3], ib3[3], cb3[3];
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            eb[u] = e; ib3[u] = jb + 1 + ii; cb3[u] = jb + 1 + cc;
            advance(e, ii, cc);
          }
          d4 x[3];
          double fa[3][4], fb[3][4];
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const bool on = eb[u] < npair;      // (off: a dummy on block (jb+1, jb+1), read only)
            const int ib = on ? ib3[u] : jb + 1, cb = on ? cb3[u] : jb + 1;
            const double* blk = sm + blk_idx(ib, cb) * 256;
            const double* la = sm + blk_idx(cb, jb) * 256;
            const double* lb = sm + blk_idx(ib, jb) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[u][r] = blk[64 * r + l];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) { fa[u][s4] = -la[64 * s4 + l]; fb[u][s4] = lb[64 * s4 + l]; }
          }
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int u = 0; u < 3; ++u) x[u] = mfma(fa[u][s4], fb[u][s4], x[u]);
#pragma unroll
          for (int u = 0; u < 3; ++u)
            if (eb[u] < npair) {
              double* blk = sm + blk_idx(ib3[u], cb3[u]) * 256;
#pragma unroll
              for (int r = 0; r < 4; ++r) blk[64 * r + l] = x[u][r];
            }
        }
      }
      // r_ib -= L(ib,jb) alpha_jb: one row per thread from rbase on (rbase >= 64) — not the wave that carries the serial chain
      if (tid >= rbase && tid - rbase >= (jb + 1) * 16 && tid - rbase < rrows) {
        const int ti_ = tid - rbase;
        const double* lb = sm + blk_idx(ti_ >> 4, jb) * 256;
        double t0 = rvec[ti_], t1 = 0.0;
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
          t0 = fma(-lb[q * 16 + (ti_ & 15)], avec[jb * 16 + q], t0);
          t1 = fma(-lb[(q + 1) * 16 + (ti_ & 15)], avec[jb * 16 + q + 1], t1);
        }
        rvec[ti_] = t0 + t1;
      }
      if (jb == 0) probe(6);
      if (w == 0 && jb + 1 < nsteps) factor16<WHBM>(sm, Wl, Wg, jb + 1, pivot_base, bad, l);      // (its block was brought up to date by this wave just above)
      if (jb == 0) probe(7);
    }
    __syncthreads();
    if (jb == 0) probe(8);
  }
}

}  // namespace agp
