// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of
// the resampling kernels: 128-bit counter, 64-bit key, ten rounds, the key bumped between rounds.  Host and device: the host form is
// what a stand-alone program checks against the published known answers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sat {

__host__ __device__ __forceinline__ uint32_t mulhi_u32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                       uint32_t (&out)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = mulhi_u32(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = mulhi_u32(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;                                   // (uniform: the ten keys of a launch are scalar work)
    k1 += W1;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the 32-bit word u as an index of 0 .. n - 1: (u * n) >> 32.  Two indices differ in probability by at most n / 2^32 relative.
__host__ __device__ __forceinline__ uint32_t index_of_word(uint32_t u, uint32_t n) { return mulhi_u32(u, n); }

}  // namespace sat
