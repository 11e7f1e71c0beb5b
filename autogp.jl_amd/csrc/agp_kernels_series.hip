// Kernel translation unit 3: the small-matrix value kernel (agp_series_kernel.hpp), behind agp_launch.hpp.
#include "agp_launch.hpp"
#include "agp_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_series() {
  const void* fns[] = {reinterpret_cast<const void*>(&k_series_logpdf<4>), reinterpret_cast<const void*>(&k_series_logpdf<8>),
                       reinterpret_cast<const void*>(&k_series_logpdf<4, true>)};
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

hipError_t launch_series_probe(hipStream_t st, const SeriesProbeArgs& sa, int grid, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (sa.n <= 0 || sa.n > SERIES_MAX_N || lds_bytes > (size_t)SERIES_LDS_BYTES) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_series_logpdf<4, true>), dim3(grid), dim3(256), lds_bytes, st, sa);      // (the evaluation stack is unused: one depth)
  return hipGetLastError();
}

}  // namespace agp
