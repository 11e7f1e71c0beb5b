// Kernel translation unit 6: the probe instantiation of the long-series value kernel (k_long_series_logpdf<4, true>,
// agp_long_series_kernel.hpp; agp_debug_long_series_factor), behind agp_launch.hpp.  A unit of its own for the reason
// agp_kernels_long_series.hip is one: the production instantiations compile as they did before the probe existed.
#include "agp_launch.hpp"
#include "agp_long_series_kernel.hpp"

namespace agp {

// lds_bytes = long_series_lds(n, 0, 0, 0): 21.5 KiB at 512 points, below the static ceiling — no attribute to raise
hipError_t launch_long_series_probe(hipStream_t st, const LongSeriesProbeArgs& la, int grid, size_t lds_bytes) {
  if (grid <= 0) return hipSuccess;
  if (la.n <= 0 || la.n > LONG_SERIES_MAX_N || lds_bytes > (size_t)(64 << 10) || la.ws == nullptr) return hipErrorInvalidValue;
  const long long nb = (la.n + BS - 1) / BS;
  if (la.ws_stride < 256 * nb * (nb + 1) / 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_long_series_logpdf<4, true>), dim3(grid), dim3(256), lds_bytes, st, la);      // (the evaluation stack is unused: one depth)
  return hipGetLastError();
}

}  // namespace agp
