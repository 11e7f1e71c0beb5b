// Kernel translation unit 5: the long-series value kernel (k_long_series_logpdf, agp_long_series_kernel.hpp), behind agp_launch.hpp.
// A unit of its own for the reason agp_kernels_series_hmc.hip is one: new instantiations beside the short-series kernels change how
// those compile.
#include "agp_launch.hpp"
#include "agp_long_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_long_series() {
  const void* fns[] = {reinterpret_cast<const void*>(&k_long_series_logpdf<4>), reinterpret_cast<const void*>(&k_long_series_logpdf<8>)};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SERIES_LDS_BYTES - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_long_series_logpdf(hipStream_t st, const LongSeriesArgs& la, int grid, int depth, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || la.ws == nullptr || la.ws_stride <= 0) return hipErrorInvalidValue;
  if (depth <= 4) hipLaunchKernelGGL(k_long_series_logpdf<4>, dim3(grid), dim3(256), lds_bytes, st, la);
  else hipLaunchKernelGGL(k_long_series_logpdf<8>, dim3(grid), dim3(256), lds_bytes, st, la);
  return hipGetLastError();
}

}  // namespace agp
