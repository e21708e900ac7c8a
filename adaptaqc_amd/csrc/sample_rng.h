// Counter-based random numbers of the shot samplers (sample.hip): Philox4x32-10 (Salmon et al.,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11).  A shot's uniform depends only on
// (seed, run, shot, site): key = (seed lo, seed hi), counter = (shot lo, shot hi, site, run).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define AQC_HD __host__ __device__
#else
#define AQC_HD
#endif

namespace aqc {

AQC_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                 uint32_t out[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// 53 bits of the first two output words as a double in [0, 1)
AQC_HD inline double sample_uniform(uint64_t seed, uint64_t run, uint64_t shot, uint32_t site) {
  uint32_t x[4];
  philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), site, (uint32_t)run, (uint32_t)seed, (uint32_t)(seed >> 32), x);
  return ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace aqc
