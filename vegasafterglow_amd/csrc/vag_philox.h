// vag_philox.h -- the counter-based draws of the device ensemble sampler (INTEGRATION.md "the device sampler"): Philox4x32-10
// (Salmon et al. 2011, the Random123 constants), the 53-bit uniform formed from two output words, and the stretch factor of the
// Goodman & Weare move.  Plain inline functions for host and device: the kernels of vag_sampler.h and a host program compiled
// with the system C++ compiler (tests/philox_check.cpp) include the same text.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define VAG_PHILOX_HD __host__ __device__
#else
#define VAG_PHILOX_HD
#endif

namespace vag {

constexpr int STRETCH_LANES = 256;  // lanes per workgroup of every sampler kernel: ceil(items / 256) groups (vag_sampler_plan.h)

// out[4] = Philox4x32-10(counter[4], key[2]); out may be counter
VAG_PHILOX_HD inline void philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;  // (the Weyl sequence of the key: bumped after every round, the last bump unused)
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the uniform in [0, 1) of two output words: 27 bits of hi, 26 of lo, exact in a double
VAG_PHILOX_HD inline double u53(uint32_t hi, uint32_t lo) {
    return (double)(((uint64_t)(hi >> 5) << 26) + (uint64_t)(lo >> 6)) * 0x1p-53;
}

// z of the stretch move from a uniform u in [0, 1): g(z) ~ 1/sqrt(z) on [1/a, a).  One fma, one multiplication, one IEEE division.
// The half-open end is kept in floating point: for the last few u below 1 the fma rounds t up to a (a = 2, u = 1 - 2^-53:
// 2 - 2^-53 ties to 2) and t t / a would be a itself; z is then the largest double below a.
VAG_PHILOX_HD inline double stretch_z(double a, double u) {
    const double t = std::fma(a - 1.0, u, 1.0);
    const double z = t * t / a;
    return z < a ? z : std::nextafter(a, 0.0);
}

// walker j of the complementary half (of `half` walkers) from an output word
VAG_PHILOX_HD inline int stretch_partner(uint32_t x, int half) { return (int)(((uint64_t)x * (uint64_t)half) >> 32); }

}  // namespace vag
