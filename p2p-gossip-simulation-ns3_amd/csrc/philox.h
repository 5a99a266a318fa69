// philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), the counter-based generator of the
// synthetic schedules (schedule_gpu.hip) and of the fanout selection (fanout_kernel.h).  Host and
// device: plain C++ when no HIP compiler reads it (the stand-alone checkers under tests/).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GOSSIP_HD __host__ __device__ __forceinline__
#else
#define GOSSIP_HD inline
#endif

namespace gossip {

constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // the key schedule's increments

// one round with the round's key
GOSSIP_HD void philox4x32_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
}

GOSSIP_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox4x32_round(c, k0, k1);
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

}  // namespace gossip
