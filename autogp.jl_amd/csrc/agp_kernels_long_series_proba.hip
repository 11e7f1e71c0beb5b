// Kernel translation unit 8: the held-out twin of the long-series value kernel (k_long_series_predict_logpdf,
// agp_long_series_kernel.hpp; agp_predict_logpdf_long_series_batch), behind agp_launch.hpp.  A unit of its own for the reason
// agp_kernels_long_series_probe.hip and agp_kernels_long_series_predict.hip are: the value, probe and predictive instantiations
// compile as they did before the twin existed (csrc/Makefile compiles every *.hip of the directory).
//
// k_long_series_predict_logpdf<D> is k_long_series_logpdf<D, false, LongSeriesProbaArgs>: the value kernel's statements on the JOINT
// points of a series — its n training points followed, without padding, by its m query points, N = n + m <= 512 — with the diagonal
// addend noise below row n and noise_pred from there on, and another read-out: both of stage 4's reductions run over the query rows
// [n, N) alone (a row in front of them contributes an exact 0.0 in its place of the fixed order), out_lp = -(m log 2 pi + 2 sum log
// L_kk + sum z_k^2) / 2 + m log|slope|, and behind stage 4's barrier the per-point terms of row n + j from alpha and the log-diagonal
// in LDS.  Every statement of its own sits behind the trait JOINT of the kernel template; no barrier is added to the block-column loop.
// With n = 0, slope 1 and noise_pred = noise the bits are the value kernel's on the series (tq, y).
// Workspace per workgroup: the value kernel's, long_series_ws_blocks(nb) blocks of 2 KiB at nb = ceil(N / 16) — 528 blocks =
// 1 081 344 bytes at 512 joint points.
// LDS: the value kernel's map at N (long_series_lds): 21 KiB + the program + 4 KiB per ChangePoint node at 512 joint points — 61 KiB
// beside 10 nodes, two workgroups per CU; 34 nodes beside a chain's program fit one workgroup's 160 KiB, 35 do not.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), D = 4 and D = 8 alike: 256 VGPRs, no AGPRs, 0 VGPRs spilled,
// scratch 0 bytes per lane, 2 waves per SIMD (__launch_bounds__(256, 2)); 168 SGPRs are kept in VGPR lanes (the value kernel: 150 —
// the twin's seven further arguments are live across the block-column loop).
// Measured (profiles/long_series_proba_perf.txt): kernels 1.17 ms against the value kernel's 1.16 ms on the concatenated series at 64
// series x (406 + 36) points x 8 particles, 0.263 against 0.258 ms at 64 x (144 + 36) x 8, 0.723 against 0.708 ms for one (406 + 36)
// series — 1 to 3 % above the same factorisation without the twin's branches; for the single series beyond the spread of the repeats.
#include "agp_launch.hpp"
#include "agp_long_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_long_series_proba() {
  const void* fns[] = {reinterpret_cast<const void*>(k_long_series_predict_logpdf<4>),
                       reinterpret_cast<const void*>(k_long_series_predict_logpdf<8>)};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SERIES_LDS_BYTES - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_long_series_predict_logpdf(hipStream_t st, const LongSeriesProbaArgs& la, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || la.ws == nullptr || la.ws_stride <= 0) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_long_series_predict_logpdf<4>, dim3(grid), dim3(256), lds_bytes, st, la);
  else hipLaunchKernelGGL(k_long_series_predict_logpdf<8>, dim3(grid), dim3(256), lds_bytes, st, la);
  return hipGetLastError();
}

}  // namespace agp
