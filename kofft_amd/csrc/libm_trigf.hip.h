// libm_trigf.hip.h -- the `sinf` / `cosf` of the libm 0.2 crate that hartley.rs:8 and window_more.rs:10 import (not Rust's std, not
// glibc, not the device's OCML), restated for the kernels (hartley_impl.hip.h) and for the host (tables.cpp: this header compiles
// with a plain C++ compiler too).  libm's sinf.rs / cosf.rs / k_sinf.rs / k_cosf.rs / rem_pio2f.rs are the musl / FreeBSD s_sinf.c,
// s_cosf.c, k_sinf.c, k_cosf.c and e_rem_pio2f.c ports: the f32 argument is widened to f64, brought into [-pi/4, pi/4] either by
// adding a multiple of pi/2 (|x| <= 9 pi/4) or by fn = round(x * 2/pi) and y = (x - fn * pio2_1) - fn * pio2_1t, and a degree-7 sine
// or degree-8 cosine polynomial is evaluated in f64 and rounded to f32 once.  Every f64 operation is one rounding in the crate's
// order and nothing may fuse (the library builds with -ffp-contract=off; no fma here); the final conversion is round-to-nearest-even.
// No Rust libm source is on the build machine: like libm_logf.hip.h this follows the published algorithm.
//
// PRECONDITION: a finite |x| >= 0x4dc90fdb (about 4.2e8) needs the crate's rem_pio2_large, which is NOT restated here; the result
// for such an argument is unspecified (libm_trigf_in_range tells; kofft_hip_libm_trigf answers KOFFT_ERR_UNSUPPORTED).  The Hartley
// angles at n <= 4096 stay below 25 736 and the window arguments below 19.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KOFFT_TRIGF_FN __host__ __device__ __forceinline__
#else
#define KOFFT_TRIGF_FN inline
#endif

#include <cstdint>

namespace kofft {
namespace trigf {

constexpr double f64_bits(uint64_t u) { return __builtin_bit_cast(double, u); }

// k_sinf.rs / k_cosf.rs: |x| <= pi/4 in f64, error below 2^-37.5
constexpr double S1 = f64_bits(0xbfc5555554cbac77ull);  // -0x15555554cbac77p-55  -0.166666666416265235595
constexpr double S2 = f64_bits(0x3f811110896efbb2ull);  //  0x111110896efbb2p-59   0.0083333293858894631756
constexpr double S3 = f64_bits(0xbf2a00f9e2cae774ull);  // -0x1a00f9e2cae774p-65  -0.000198393348360966317347
constexpr double S4 = f64_bits(0x3ec6cd878c3b46a7ull);  //  0x16cd878c3b46a7p-71   0.0000027183114939898219064
constexpr double C0 = f64_bits(0xbfdffffffd0c5e81ull);  // -0x1ffffffd0c5e81p-54  -0.499999997251031003120
constexpr double C1 = f64_bits(0x3fa55553e1053a42ull);  //  0x155553e1053a42p-57   0.0416666233237390631894
constexpr double C2 = f64_bits(0xbf56c087e80f1e27ull);  // -0x16c087e80f1e27p-62  -0.00138867637746099294692
constexpr double C3 = f64_bits(0x3ef99342e0ee5069ull);  //  0x199342e0ee5069p-68   0.0000243904487962774090654
static_assert(S1 == -0x15555554cbac77p-55 && S2 == 0x111110896efbb2p-59 && S3 == -0x1a00f9e2cae774p-65 && S4 == 0x16cd878c3b46a7p-71, "k_sinf");
static_assert(C0 == -0x1ffffffd0c5e81p-54 && C1 == 0x155553e1053a42p-57 && C2 == -0x16c087e80f1e27p-62 && C3 == 0x199342e0ee5069p-68, "k_cosf");
// rem_pio2f.rs
constexpr double TOINT = f64_bits(0x4338000000000000ull);     // 1.5 * 2^52
constexpr double INV_PIO2 = f64_bits(0x3fe45f306dc9c883ull);  // 6.36619772367581382433e-01: 53 bits of 2 / pi
constexpr double PIO2_1 = f64_bits(0x3ff921fb50000000ull);    // 1.57079631090164184570e+00: the first 25 bits of pi / 2
constexpr double PIO2_1T = f64_bits(0x3e5110b4611a6263ull);   // 1.58932547735281966916e-08: pi / 2 - PIO2_1
static_assert(TOINT == 1.5 * 4503599627370496.0 && INV_PIO2 == 6.36619772367581382433e-01 && PIO2_1 == 1.57079631090164184570e+00 &&
                  PIO2_1T == 1.58932547735281966916e-08,
              "rem_pio2f");
// sinf.rs / cosf.rs: k * FRAC_PI_2 as f64, one rounding each (k = 2, 4 are exact doublings)
constexpr double FRAC_PI_2 = f64_bits(0x3ff921fb54442d18ull);
static_assert(FRAC_PI_2 == 1.57079632679489661923132169163975144, "core::f64::consts::FRAC_PI_2");
constexpr double P1 = 1.0 * FRAC_PI_2, P2 = 2.0 * FRAC_PI_2, P3 = 3.0 * FRAC_PI_2, P4 = 4.0 * FRAC_PI_2;

KOFFT_TRIGF_FN float k_sinf(double x)
{
    const double z = x * x;
    const double w = z * z;
    const double r = S3 + z * S4;
    const double s = z * x;
    return (float)((x + s * (S1 + z * S2)) + s * w * r);
}

KOFFT_TRIGF_FN float k_cosf(double x)
{
    const double z = x * x;
    const double w = z * z;
    const double r = C2 + z * C3;
    return (float)(((1.0 + z * C0) + w * C1) + (w * z) * r);
}

// rem_pio2f, the medium range (ix < 0x4dc90fdb): n = the multiple of pi / 2 taken out, *y the remainder
KOFFT_TRIGF_FN int rem_pio2f_medium(double x64, double *y)
{
    const double fn = (x64 * INV_PIO2 + TOINT) - TOINT;
    *y = (x64 - fn * PIO2_1) - fn * PIO2_1T;
    return (int)fn;  // |fn| < 2.7e8: in range
}

}  // namespace trigf

// true where libm_sinf / libm_cosf restate the crate: everything but a finite |x| >= 0x4dc90fdb
KOFFT_TRIGF_FN bool libm_trigf_in_range(float x)
{
    const uint32_t ix = __builtin_bit_cast(uint32_t, x) & 0x7fffffffu;
    return ix < 0x4dc90fdbu || ix >= 0x7f800000u;
}

KOFFT_TRIGF_FN float libm_sinf(float x)
{
    using namespace trigf;
    const double x64 = (double)x;
    const uint32_t bits = __builtin_bit_cast(uint32_t, x);
    const bool sign = (bits >> 31) != 0;
    const uint32_t ix = bits & 0x7fffffffu;
    if (ix <= 0x3f490fdau) {               // |x| ~<= pi/4
        if (ix < 0x39800000u) return x;    // |x| < 2^-12
        return k_sinf(x64);
    }
    if (ix <= 0x407b53d1u) {      // |x| ~<= 5 pi/4
        if (ix <= 0x4016cbe3u) {  // |x| ~<= 3 pi/4
            if (sign) return -k_cosf(x64 + P1);
            return k_cosf(x64 - P1);
        }
        return k_sinf(sign ? -(x64 + P2) : -(x64 - P2));
    }
    if (ix <= 0x40e231d5u) {      // |x| ~<= 9 pi/4
        if (ix <= 0x40afeddfu) {  // |x| ~<= 7 pi/4
            if (sign) return k_cosf(x64 + P3);
            return -k_cosf(x64 - P3);
        }
        return k_sinf(sign ? x64 + P4 : x64 - P4);
    }
    if (ix >= 0x7f800000u) return x - x;  // sin(inf or NaN) is NaN
    double y;
    const int n = rem_pio2f_medium(x64, &y);
    switch (n & 3) {
    case 0: return k_sinf(y);
    case 1: return k_cosf(y);
    case 2: return k_sinf(-y);
    default: return -k_cosf(y);
    }
}

KOFFT_TRIGF_FN float libm_cosf(float x)
{
    using namespace trigf;
    const double x64 = (double)x;
    const uint32_t bits = __builtin_bit_cast(uint32_t, x);
    const bool sign = (bits >> 31) != 0;
    const uint32_t ix = bits & 0x7fffffffu;
    if (ix <= 0x3f490fdau) {                 // |x| ~<= pi/4
        if (ix < 0x39800000u) return 1.0f;   // |x| < 2^-12
        return k_cosf(x64);
    }
    if (ix <= 0x407b53d1u) {     // |x| ~<= 5 pi/4
        if (ix > 0x4016cbe3u) {  // |x| ~> 3 pi/4
            return -k_cosf(sign ? x64 + P2 : x64 - P2);
        }
        if (sign) return k_sinf(x64 + P1);
        return k_sinf(P1 - x64);
    }
    if (ix <= 0x40e231d5u) {     // |x| ~<= 9 pi/4
        if (ix > 0x40afeddfu) {  // |x| ~> 7 pi/4
            return k_cosf(sign ? x64 + P4 : x64 - P4);
        }
        if (sign) return k_sinf(-x64 - P3);
        return k_sinf(x64 - P3);
    }
    if (ix >= 0x7f800000u) return x - x;  // cos(inf or NaN) is NaN
    double y;
    const int n = rem_pio2f_medium(x64, &y);
    switch (n & 3) {
    case 0: return k_cosf(y);
    case 1: return k_sinf(-y);
    case 2: return -k_cosf(y);
    default: return k_sinf(y);
    }
}

}  // namespace kofft
