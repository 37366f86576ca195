// libm_logf.hip.h -- the `logf` of the libm 0.2 crate that cepstrum.rs:9 imports (not Rust's std, not glibc, not the device's
// OCML), restated for the kernels and, through tools/ubench_logf.hip, for the host.  libm's logf.rs is the musl / FreeBSD e_logf.c
// port, all in f32: the argument is reduced to 2^k * (1 + f) with 1 + f in [sqrt(2)/2, sqrt(2)), then
//   s = f / (2 + f);  log(1 + f) = f - hfsq + s * (hfsq + R(s^2)),  R a degree-4 polynomial in s^2 (LG1 .. LG4).
// Every operation is one f32 rounding in the crate's order: the division is the correctly rounded one (HIP's default without
// fast-math; not __fdividef, not a reciprocal), and nothing may fuse (the library builds with -ffp-contract=off; no fmaf here).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kofft {

__host__ __device__ __forceinline__ float libm_logf(float x)
{
    constexpr float ln2_hi = __builtin_bit_cast(float, 0x3f317180u);  // 6.9313812256e-01
    constexpr float ln2_lo = __builtin_bit_cast(float, 0x3717f7d1u);  // 9.0580006145e-06
    constexpr float lg1 = __builtin_bit_cast(float, 0x3f2aaaaau);     // 0.66666662693
    constexpr float lg2 = __builtin_bit_cast(float, 0x3eccce13u);     // 0.40000972152
    constexpr float lg3 = __builtin_bit_cast(float, 0x3e91e9eeu);     // 0.28498786688
    constexpr float lg4 = __builtin_bit_cast(float, 0x3e789e26u);     // 0.24279078841
    constexpr float x1p25 = __builtin_bit_cast(float, 0x4c000000u);   // 2^25

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
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * (lg2 + w * lg4);
    const float t2 = z * (lg1 + w * lg3);
    const float r = t2 + t1;
    const float hfsq = 0.5f * f * f;
    const float dk = (float)k;
    return s * (hfsq + r) + dk * ln2_lo - hfsq + f + dk * ln2_hi;
}

}  // namespace kofft
