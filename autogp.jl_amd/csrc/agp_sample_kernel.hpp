// Posterior predictive samples (agp_predict_sample_batch; rand(predict_mvn(model, ds), N), src/api.jl:497-522) on the joint factor
// that agp_predict_logpdf_batch's pass leaves in A: its query block is L22 = chol(Sigma*), its query-row block L21 = K21 L11^-T, and
// the forward solve leaves a = L11^-1 (x - mu1) in the vector, so every sample is one read-out of the query tile rows,
//     x_s = mu2 + [L21 L22] [a; z_s]       (mu* = mu2 + L21 a;  L22 z_s ~ N(0, Sigma*)),
// then the raw-space transform of predict_mvn, x_raw = (mu* - b) / a + (L22 z) / |a|, evaluated as (mu2 + L21 a + sign(a) L22 z - b) / a
// (the sign flip of z is exact).
//
// k_philox_normals: Z (row i, column j) = ndtri(u) of word i % 4 of the Philox4x64-10 block (i / 4, s_j, 1, 0) under the key (seed, 0),
// or the caller's z[s_j * m + i]; padding rows and columns 0.
//
// k_pred_sample: one workgroup per (group of up to SMP_G samples of one particle, query tile row i).  The MFMA operands are swapped as in
// the update GEMM of the factorisation (agp_chol_kernel.hpp), so that the accumulator's lane % 16 runs along the tile's rows, which are
// contiguous in the column-major tile and in the output column: D'(sample, row) = sum_k [a 1^T; Z](k, sample) L(row, k) on
// v_mfma_f64_16x16x4, wave w owning tile rows [32 w, 32 w + 32) of all SMP_G samples (2 x 2 accumulators).  The K loop runs over tile
// columns 0 .. nt1 + i: the training columns multiply a (the same for every sample: one accumulator pair, copied to the second sample
// block), the query columns Z; of the diagonal tile only the lower triangle counts (the upper part, which holds NaN on a poisoned
// engine, is replaced by 0 with a select) and the wave stops after its own last row.  Each output element is one accumulation chain in
// a fixed order over k that does not depend on the other samples of its workgroup: x[:, s] does not depend on S, on which samples
// share a group, or on the chunking.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "agp_args.hpp"
#include "agp_chol_kernel.hpp"
#include "agp_ndtri.hpp"
#include "agp_philox.hpp"

namespace agp {

__global__ __launch_bounds__(256) void k_philox_normals(SampleNormArgs a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.ldz) return;
  const bool live = j < a.S;
  const long long s = live ? a.col[j] : 0;
  for (int i4 = blockIdx.y; 4 * i4 < a.m_pad; i4 += gridDim.y) {
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (live && 4 * i4 < a.m) {
      if (a.zin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 4 * i4 + r;
          if (i < a.m) z[r] = a.zin[s * a.m + i];
        }
      } else {
        const Philox4 b = philox4x64_10((uint64_t)i4, (uint64_t)s, 1, 0, a.seed, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * i4 + r < a.m) z[r] = ndtri(philox_uniform(b.w[r]));
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) a.Z[(long long)(4 * i4 + r) * a.ldz + j] = z[r];
  }
}

__global__ __launch_bounds__(256) void k_pred_sample(SampleReadArgs a) {
  const int32_t* g = a.grp + 4 * (long long)blockIdx.x;
  const int q = g[0], j0 = g[1], cnt = g[2];
  const int i = blockIdx.y, I = a.nt1 + i;
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = l & 15, lq = l >> 4;
  const int r0 = 32 * w;                   // this wave's tile rows: r0 + [0, 32)
  const double* __restrict__ Ap = a.A + (long long)q * a.strideA;
  const double* __restrict__ av = a.vec + (long long)q * a.ldv;
  const int g0 = i * NB + r0 + l15, g1 = g0 + 16;      // the lane's query rows (accumulator columns) of the two row blocks
  const double mu0 = (a.mu2 && g0 < a.m) ? a.mu2[g0] : 0.0, mu1 = (a.mu2 && g1 < a.m) ? a.mu2[g1] : 0.0;
  d4 c00 = {mu0, mu0, mu0, mu0}, c01 = {mu1, mu1, mu1, mu1};      // c[sample block][row block]
  // training columns: L21 a, the same for every sample
  for (int J = 0; J < a.nt1; ++J) {
    const double* __restrict__ T = Ap + tile_off(I, J) + r0 + l15;
    const double* __restrict__ aj = av + J * NB + lq;
#pragma unroll 8
    for (int k = 0; k < NB; k += 4) {
      const double x = aj[k];
      const double b0 = T[(long long)(k + lq) * NB], b1 = T[(long long)(k + lq) * NB + 16];
      c00 = mfma(x, b0, c00);
      c01 = mfma(x, b1, c01);
    }
  }
  d4 c10 = c00, c11 = c01;
  // query columns: L22 z (sign(slope) z), lower triangle of the diagonal tile only
  for (int J = a.nt1; J <= I; ++J) {
    const bool diag = J == I;
    const int kend = diag ? r0 + 32 : NB;
    const double* __restrict__ T = Ap + tile_off(I, J) + r0 + l15;
    const double* __restrict__ zr = a.Z + (long long)(J - a.nt1) * NB * a.ldz + j0 + l15;
    for (int k0 = 0; k0 < kend; k0 += 16) {      // (kend is a multiple of 32)
#pragma unroll
      for (int k = k0; k < k0 + 16; k += 4) {
        const int kq = k + lq;
        double b0 = T[(long long)kq * NB], b1 = T[(long long)kq * NB + 16];
        if (diag) {
          b0 = kq <= r0 + l15 ? b0 : 0.0;
          b1 = kq <= r0 + 16 + l15 ? b1 : 0.0;
        }
        const double z0 = a.zsign * zr[(long long)kq * a.ldz], z1 = a.zsign * zr[(long long)kq * a.ldz + 16];
        c00 = mfma(z0, b0, c00);
        c01 = mfma(z0, b1, c01);
        c10 = mfma(z1, b0, c10);
        c11 = mfma(z1, b1, c11);
      }
    }
  }
  // accumulator (lane, reg t): sample 4 t + lane / 16 of its block, row lane % 16 of its block
  auto put = [&](const d4& c, int sb, int gr) {
    if (gr >= a.m) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int jl = 16 * sb + 4 * t + lq;
      if (jl < cnt) a.out[(long long)a.col[j0 + jl] * a.m + gr] = (c[t] - a.intercept) / a.slope;
    }
  };
  put(c00, 0, g0); put(c01, 0, g1); put(c10, 1, g0); put(c11, 1, g1);
}

}  // namespace agp
