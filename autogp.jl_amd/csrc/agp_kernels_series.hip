// Kernel translation unit 3: the small-matrix value kernel, its value-and-gradient twin, its predictive twin and the latter's
// held-out, sampling and decomposition twins (agp_series_kernel.hpp), behind agp_launch.hpp.
#include "agp_launch.hpp"
#include "agp_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_series() {
  const void* fns[] = {reinterpret_cast<const void*>(&k_series_logpdf<4>), reinterpret_cast<const void*>(&k_series_logpdf<8>),
                       reinterpret_cast<const void*>(&k_series_logpdf<4, true>),
                       reinterpret_cast<const void*>(&k_series_logpdf_grad<4, 16>), reinterpret_cast<const void*>(&k_series_logpdf_grad<4, 64>),
                       reinterpret_cast<const void*>(&k_series_logpdf_grad<8, 64>),
                       reinterpret_cast<const void*>(&k_series_predict<4>), reinterpret_cast<const void*>(&k_series_predict<8>),
                       reinterpret_cast<const void*>(&k_series_predict_logpdf<4>), reinterpret_cast<const void*>(&k_series_predict_logpdf<8>),
                       reinterpret_cast<const void*>(&k_series_predict_sample<4>), reinterpret_cast<const void*>(&k_series_predict_sample<8>),
                       reinterpret_cast<const void*>(&k_series_predict_sum<4>), reinterpret_cast<const void*>(&k_series_predict_sum<8>)};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SERIES_LDS_BYTES - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_series_logpdf(hipStream_t st, const SeriesArgs& sa, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_series_logpdf<4>, dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL(k_series_logpdf<8>, dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_logpdf_grad(hipStream_t st, const SeriesGradArgs& sa, int grid, int depth, int tape, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || tape > 64 || (depth > 4 && tape <= 16)) return hipErrorInvalidValue;
  if (tape <= 16) hipLaunchKernelGGL((k_series_logpdf_grad<4, 16>), dim3(grid), dim3(256), lds_bytes, st, sa);
  else if (depth <= 4) hipLaunchKernelGGL((k_series_logpdf_grad<4, 64>), dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL((k_series_logpdf_grad<8, 64>), dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_predict(hipStream_t st, const SeriesPredArgs& sa, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_series_predict<4>, dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL(k_series_predict<8>, dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_predict_sum(hipStream_t st, const SeriesSumArgs& sa, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || sa.M < 1 || sa.nq < 0) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_series_predict_sum<4>, dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL(k_series_predict_sum<8>, dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_predict_logpdf(hipStream_t st, const SeriesProbaArgs& sa, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_series_predict_logpdf<4>, dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL(k_series_predict_logpdf<8>, dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_predict_sample(hipStream_t st, const SeriesSampleArgs& sa, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_series_predict_sample<4>, dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL(k_series_predict_sample<8>, dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

hipError_t launch_series_sample_fill(hipStream_t st, const SeriesSampleFillArgs& a) {
  if (a.S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_series_sample_fill, dim3(a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_series_probe(hipStream_t st, const SeriesProbeArgs& sa, int grid, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (sa.n <= 0 || sa.n > SERIES_MAX_N || lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_series_logpdf<4, true>), dim3(grid), dim3(256), lds_bytes, st, sa);      // (the evaluation stack is unused: one depth)
  return hipGetLastError();
}

}  // namespace agp
