// ao_dir.hpp — the ambient-occlusion frames' direction of occlusion ray k of point i (rray.h
// RR_HAS_AO holds the definition).  Header-only and __host__ __device__: ao_pairs_kernel (render_ao.inc) and the host
// entry rr_ao_directions (api.cpp) call the same functions, so the definition is testable without a device.  Plain
// f64 in exactly the order written, compiled without contraction (-ffp-contract=off); the integer mixes are
// device_core.inc's splitmix64 / lowbias32 / jitter_base, restated here because those are device-only.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RR_AO_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_AO_HD inline
#endif

namespace rr {

RR_AO_HD uint64_t ao_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
RR_AO_HD uint32_t ao_lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// jitter_base(seed, i, path 0): one 64-bit mix per point
RR_AO_HD uint32_t ao_base(uint64_t seed, uint64_t i) { return (uint32_t)(ao_splitmix64(seed ^ ao_splitmix64(i)) >> 32); }
// u(k, j) = lowbias32(base ^ ((k << 21) | j)) * 2^-32 in [0, 1): jitter_value(base, k, j >> 1, j & 1)
RR_AO_HD double ao_u(uint32_t base, uint32_t k, uint32_t j) {
    return (double)ao_lowbias32(base ^ ((k << 21) | j)) * (1.0 / 4294967296.0);
}

// w of occlusion ray k around the unit normal N.  All eight rejection rounds run whatever they find (sixteen 32-bit
// hashes), so a wave's lanes do not diverge; the first pair inside the unit disc is kept.  Malley's method lifts the
// disc point onto the hemisphere (cosine-weighted, w . N = c >= 0 up to rounding); the frame is Duff et al.'s
// branch-free basis, whose divisor s + N.z has magnitude in [1, 2] for every unit N (s is N.z's sign, -0.0 included).
RR_AO_HD void ao_direction(uint32_t base, uint32_t k, const double N[3], double w[3]) {
    double A = 0.0, B = 0.0;
    bool found = false;
#pragma unroll
    for (uint32_t a = 0; a < 8u; ++a) {
        const double ca = 2.0 * ao_u(base, k, 2u * a) - 1.0;
        const double cb = 2.0 * ao_u(base, k, 2u * a + 1u) - 1.0;
        const bool in = ca * ca + cb * cb <= 1.0;
        if (!found && in) {
            A = ca;
            B = cb;
        }
        found = found || in;
    }
    const double c = sqrt(1.0 - (A * A + B * B));
    const double s = copysign(1.0, N[2]);
    const double q = -1.0 / (s + N[2]);
    const double b = (N[0] * N[1]) * q;
    const double T[3] = {1.0 + (s * (N[0] * N[0])) * q, s * b, -(s * N[0])};
    const double Bv[3] = {b, s + (N[1] * N[1]) * q, -N[1]};
    for (int r = 0; r < 3; ++r) w[r] = (A * T[r] + B * Bv[r]) + c * N[r];
}

}  // namespace rr
