// Kernel translation unit 7: the predictive twin of the long-series value kernel (k_long_series_predict, agp_long_series_kernel.hpp;
// agp_predict_long_series_batch, agp_predict_quantile_long_series_batch), behind agp_launch.hpp.  A unit of its own for the reason
// agp_kernels_long_series_probe.hip is one: the value kernel's instantiations compile as they did before the twin existed.
//
// k_long_series_predict<D> is long_series_body on LongSeriesPredArgs: stages 1 - 4 are the value kernel's statements (the value's
// bits are that kernel's), factor16<true> also leaves W(j) = L(j, j)^-1 behind the triangle, and stage P — the posterior at the
// series' own query times — runs behind stage 4's barrier without another.  Rounds of LONG_PRED_C = 2 query blocks per wave: the
// two chains share the L(j, k) operand of long_update.  One chain per wave was not built separately — every measured shape has at
// most four query blocks, one per wave, where a round holds a single chain whatever LONG_PRED_C is; four chains per wave (768
// table entries per ChangePoint node) would put ten nodes at 512 points at 81 KiB and cost the second workgroup of a CU.
// Workspace per workgroup at 512 points (nb = 32): 528 blocks of the triangle + 292 of the eight scratch rows in the triangle's
// packing (8 x 33 are used; row pointers for long_update would save 28 blocks, 56 KiB of 1.7 MiB, and were not worth a second copy
// of its loop) + 32 inverses = 852 blocks of 2 KiB = 1 744 896 bytes, whatever the number of query times.
// LDS at 512 points: 21.5 KiB + the program + 5 KiB per ChangePoint node (LONG_PRED_SIG_STRIDE = 640 entries) — 71.5 KiB beside 10
// nodes, so two workgroups share a CU as in the value kernel.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), D = 4 / 8: 256 VGPRs, no AGPRs, 0 VGPRs spilled, scratch 0 bytes per
// lane, 2 waves per SIMD (__launch_bounds__(256, 2)); 221 / 223 SGPRs are kept in VGPR lanes (the value kernel: 150).
// Measured (profiles/long_series_predict_perf.txt): kernels 1.63 ms against the value kernel's 1.22 ms at 64 series x 442 points x 8
// particles with 36 queries, 1.82 against 1.35 ms at 16 x 512 x 18 with 64 — three or four query blocks, one per wave, each walking
// the block columns alone.  Whether a second workgroup per CU still fits: it does (71.5 KiB, 2 waves per SIMD); not measured against
// a one-workgroup build.
#include "agp_launch.hpp"
#include "agp_long_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_long_series_predict() {
  const void* fns[] = {reinterpret_cast<const void*>(k_long_series_predict<4>), reinterpret_cast<const void*>(k_long_series_predict<8>)};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SERIES_LDS_BYTES - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_long_series_predict(hipStream_t st, const LongSeriesPredArgs& la, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || la.ws == nullptr || la.ws_stride <= 0) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_long_series_predict<4>, dim3(grid), dim3(256), lds_bytes, st, la);
  else hipLaunchKernelGGL(k_long_series_predict<8>, dim3(grid), dim3(256), lds_bytes, st, la);
  return hipGetLastError();
}

}  // namespace agp
