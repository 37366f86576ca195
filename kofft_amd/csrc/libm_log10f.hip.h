// libm_log10f.hip.h -- the `log10f` of the libm 0.2 crate (the musl / FreeBSD e_log10f.c port, all in f32), the sibling of
// libm_logf.hip.h: what a build of the reference without a platform libm computes where visual/spectrogram.rs calls `.log10()`.
// (With `std` the reference calls the platform's log10f, so its own bytes differ from platform to platform; this one is the
// contract of DESIGN 5.22.)  The argument reduction, the special cases and LG1 .. LG4 are those of libm_logf; then
//   hi = (f - hfsq) with its low 12 bits cleared, lo = the rest, and the sum of five products below, left to right.
// Every operation is one f32 rounding in the crate's order: the division is the correctly rounded one, nothing may fuse (the
// library builds with -ffp-contract=off; no fmaf here).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kofft {

__host__ __device__ __forceinline__ float libm_log10f(float x)
{
    constexpr float ivln10hi = __builtin_bit_cast(float, 0x3ede6000u);   // 4.3432617188e-01
    constexpr float ivln10lo = __builtin_bit_cast(float, 0xb804ead9u);   // -3.1689971365e-05
    constexpr float log10_2hi = __builtin_bit_cast(float, 0x3e9a2080u);  // 3.0102920532e-01
    constexpr float log10_2lo = __builtin_bit_cast(float, 0x355427dbu);  // 7.9034151668e-07
    constexpr float lg1 = __builtin_bit_cast(float, 0x3f2aaaaau);        // 0.66666662693
    constexpr float lg2 = __builtin_bit_cast(float, 0x3eccce13u);        // 0.40000972152
    constexpr float lg3 = __builtin_bit_cast(float, 0x3e91e9eeu);        // 0.28498786688
    constexpr float lg4 = __builtin_bit_cast(float, 0x3e789e26u);        // 0.24279078841
    constexpr float x1p25 = __builtin_bit_cast(float, 0x4c000000u);      // 2^25

    uint32_t ix = __builtin_bit_cast(uint32_t, x);
    int k = 0;
    if (ix < 0x00800000u || (ix >> 31) != 0) {  // x < 2^-126, or the sign bit
        if ((ix << 1) == 0) return -1.0f / (x * x);  // log(+-0) = -inf
        if ((ix >> 31) != 0) return (x - x) / 0.0f;  // log(-x) = NaN
        k -= 25;  // subnormal: scale up
        x *= x1p25;
        ix = __builtin_bit_cast(uint32_t, x);
    } else if (ix >= 0x7f800000u) {
        return x;  // +inf, NaN
    } else if (ix == 0x3f800000u) {
        return 0.0f;
    }
    // reduce x into [sqrt(2)/2, sqrt(2))
    ix += 0x3f800000u - 0x3f3504f3u;
    k += (int)(ix >> 23) - 0x7f;
    ix = (ix & 0x007fffffu) + 0x3f3504f3u;
    x = __builtin_bit_cast(float, ix);

    const float f = x - 1.0f;
    const float hfsq = 0.5f * f * f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * (lg2 + w * lg4);
    const float t2 = z * (lg1 + w * lg3);
    const float r = t2 + t1;
    const float hi = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f - hfsq) & 0xfffff000u);
    const float lo = f - hi - hfsq + s * (hfsq + r);
    const float dk = (float)k;
    return dk * log10_2lo + (lo + hi) * ivln10lo + lo * ivln10hi + hi * ivln10hi + dk * log10_2hi;
}

}  // namespace kofft
