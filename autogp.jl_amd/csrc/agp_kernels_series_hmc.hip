// Kernel translation unit 4: the HMC twin of the small-matrix kernels (k_series_hmc, agp_series_kernel.hpp), behind agp_launch.hpp.
// A unit of its own: with these instantiations beside them the other series kernels compile to other instruction streams (the
// inliner weighs the call sites of a module together); alone in agp_kernels_series.hip they are what they were.
#include "agp_launch.hpp"
#define AGP_SERIES_TEMPLATES_ONLY
#include "agp_series_kernel.hpp"

namespace agp {

hipError_t kernels_init_series_hmc() {
  const void* fns[] = {reinterpret_cast<const void*>(&k_series_hmc<4, 16>), reinterpret_cast<const void*>(&k_series_hmc<4, 64>),
                       reinterpret_cast<const void*>(&k_series_hmc<8, 64>)};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SERIES_LDS_BYTES - (int)fa.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_series_hmc(hipStream_t st, const SeriesHmcArgs& sa, int grid, int depth, int tape, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (lds_bytes > (size_t)SERIES_LDS_BYTES || tape > 64 || (depth > 4 && tape <= 16)) return hipErrorInvalidValue;
  if (tape <= 16) hipLaunchKernelGGL((k_series_hmc<4, 16>), dim3(grid), dim3(256), lds_bytes, st, sa);
  else if (depth <= 4) hipLaunchKernelGGL((k_series_hmc<4, 64>), dim3(grid), dim3(256), lds_bytes, st, sa);
  else hipLaunchKernelGGL((k_series_hmc<8, 64>), dim3(grid), dim3(256), lds_bytes, st, sa);
  return hipGetLastError();
}

}  // namespace agp
