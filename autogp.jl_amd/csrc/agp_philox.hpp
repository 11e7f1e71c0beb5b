// Counter-based random numbers for posterior predictive sampling (agp_predict_sample_batch), host and device: Philox4x64-10 (Salmon,
// Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC 2011) with the round constants of Random123 — the generator
// numpy.random.Philox implements, against which tests/test_predict_sample_cpu.py pins this header.
//
// A block is the 4 x 64-bit output of one counter (c0, c1, c2, c3) under the key (seed, 0).  A 64-bit word w gives the uniform
//     u = ((w >> 11) + 0.5) * 2^-53        (fp64, round to nearest),
// which lies in (0, 1) except for the one word whose sum rounds to 2^53: that u is taken as 1 - 2^-53 (agp_philox_uniform).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AGP_PHILOX_FN __host__ __device__ inline
#else
#define AGP_PHILOX_FN inline
#endif

namespace agp {

struct Philox4 {
  uint64_t w[4];
};

AGP_PHILOX_FN uint64_t philox_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

AGP_PHILOX_FN Philox4 philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1) {
  const uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  const uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
  for (int r = 0; r < 10; ++r) {
    if (r > 0) { k0 += W0; k1 += W1; }
    const uint64_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
    const uint64_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
    const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

AGP_PHILOX_FN double philox_uniform(uint64_t w) {
  const double u = ((double)(w >> 11) + 0.5) * 0x1.0p-53;
  return u < 1.0 ? u : 1.0 - 0x1.0p-53;
}

}  // namespace agp
