// resample_plan.h -- the index arithmetic of the polyphase resampler.  Output m of a row sits at up-sampled time
// t = t0 + m * down; its phase is p = t mod up, its newest sample i0 = t div up, and its terms are h[p + j * up] * x[i0 - j] for
// j = 0, 1, .. while p + j * up < nh, of which those with 0 <= i0 - j < nx exist.  The tiled kernel gives a workgroup a tile of `tile`
// consecutive outputs of one row: the samples s_first .. s_first + s_count - 1 it stages, the phase and the sample of every output
// relative to the tile's first, the terms per phase, the LDS footprint and the route decision are all here.  Arithmetic only, no HIP
// header: the kernels (resample_impl.hip.h) and the host (k_resample_f32.hip) call these functions, and
// tests/cpp/sanitize_resample_plan.cpp includes this file alone and compares them with an enumeration of every term.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define KOFFT_PLAN_HD __host__ __device__ inline
#else
#define KOFFT_PLAN_HD inline
#endif

namespace kofft {
namespace host {

constexpr unsigned kResampleThreads = 256;             // threads of a workgroup of either kernel
constexpr unsigned kResampleTile = 1024;               // T: the most outputs of one tile of the tiled kernel (resample_tile_outputs)
constexpr unsigned long long kResampleLdsWords = 13312;  // the tiled kernel's LDS budget in floats: 52 KiB, three workgroups of 160 KiB

// the terms of phase p: the j with p + j * up < nh (U: 64 bits, or 32 where nh and up fit them)
template <typename U>
KOFFT_PLAN_HD U resample_terms(U nh, U up, U p)
{
    return p < nh ? (U)((nh - 1 - p) / up + 1) : (U)0;
}

// J: the terms of phase 0, the most any phase has (nh >= 1)
KOFFT_PLAN_HD unsigned long long resample_max_terms(unsigned long long nh, unsigned long long up) { return (nh - 1) / up + 1; }

// The floats of one phase's row of the phase-major tap table hp[p][j] = h[p + j * up]: J made odd, so that lanes whose phases differ by
// d read banks d * stride apart, distinct for every d below the number of banks.
KOFFT_PLAN_HD unsigned long long resample_tap_stride(unsigned long long terms) { return terms | 1; }

// The terms of an output that exist: j in [*jlo, *jhi) of its phase's `cnt` terms, those with 0 <= i0 - j < nx.  Both at most cnt.
KOFFT_PLAN_HD void resample_term_range(unsigned long long i0, unsigned long long nx, unsigned long long cnt, unsigned long long *jlo,
                                       unsigned long long *jhi)
{
    const unsigned long long lo = i0 >= nx ? i0 - (nx - 1) : 0;  // (i0 - j <= nx - 1)
    const unsigned long long hi = i0 < cnt ? i0 + 1 : cnt;        // (i0 - j >= 0)
    *jlo = lo < hi ? lo : hi;
    *jhi = hi;
}

// The most by which i0 grows over a tile: i0(last) - i0(first) for the worst first phase (up - 1).  Saturates.
KOFFT_PLAN_HD unsigned long long resample_tile_span(unsigned long long up, unsigned long long down, unsigned long long tile)
{
    unsigned long long a = 0;
    if (__builtin_mul_overflow(tile - 1, down, &a) || __builtin_add_overflow(a, up - 1, &a)) return ~0ULL;
    return a / up;
}

// The LDS footprint of the tiled kernel in floats: `up` tap rows of the padded stride, then span + J samples.  Saturates.
KOFFT_PLAN_HD unsigned long long resample_lds_words(unsigned long long nh, unsigned long long up, unsigned long long down, unsigned long long tile)
{
    const unsigned long long J = resample_max_terms(nh, up), span = resample_tile_span(up, down, tile);
    unsigned long long taps = 0, w = 0;
    if (__builtin_mul_overflow(up, resample_tap_stride(J), &taps) || __builtin_add_overflow(taps, span, &w) ||
        __builtin_add_overflow(w, J, &w))
        return ~0ULL;
    return w;
}

// Whether a shape can run the tiled kernel at all: the footprint inside the budget.  (Then up <= 13312 and the largest offset of an
// output from its tile's first time, r_first + (tile - 1) * down < (span + 1) * up, stays far below 2^32: the kernel's 32-bit walk.)
KOFFT_PLAN_HD bool resample_fits(unsigned long long nh, unsigned long long up, unsigned long long down)
{
    return resample_lds_words(nh, up, down, kResampleTile) <= kResampleLdsWords;
}

// The route of a default context (kofft_hip_resample_route): 1 the tiled kernel, 0 the plain one.  Monotone in nh for fixed up and
// down: the footprint only grows with nh, and so does the second condition.  The rule is the measured one of DESIGN.md 5.28.
KOFFT_PLAN_HD int resample_route(unsigned long long nh, unsigned long long up, unsigned long long down)
{
    return resample_fits(nh, up, down) ? 1 : 0;
}

// One tile: outputs m0 .. m0 + n - 1 of a row (n >= 1), the first at time t_first = t0 + m0 * down.
struct ResampleTile {
    unsigned long long q_first;  // i0 of the first output
    unsigned r_first;            // its phase
    long long s_first;           // the first sample the tile's terms name, i0(first) - J + 1: negative near the row's start
    unsigned long long s_count;  // samples s_first .. i0(last)
};

KOFFT_PLAN_HD ResampleTile resample_tile(unsigned long long t0, unsigned long long m0, unsigned long long n, unsigned long long up,
                                         unsigned long long down, unsigned long long J)
{
    const unsigned long long t_first = t0 + m0 * down, t_last = t_first + (n - 1) * down;
    ResampleTile tl;
    tl.q_first = t_first / up;
    tl.r_first = (unsigned)(t_first % up);
    tl.s_first = (long long)tl.q_first - (long long)(J - 1);
    tl.s_count = t_last / up - tl.q_first + J;
    return tl;
}

// Output dm of a tile (0 <= dm < n): its phase and its newest sample as an offset from q_first, from the 32-bit offset
// r_first + dm * down of its time.  The sample's place in the staged run is *di + J - 1.
KOFFT_PLAN_HD void resample_output(unsigned r_first, unsigned dm, unsigned up, unsigned down, unsigned *p, unsigned *di)
{
    const unsigned delta = r_first + dm * down;
    *di = delta / up;
    *p = delta - *di * up;
}

// Whether the outputs dm, dm + lanes, dm + 2 lanes, .. of a tile share their phase: lanes * down is a multiple of up.  Their newest
// samples are then lanes * down / up apart, and a thread that owns them reads every tap once for all of them.
KOFFT_PLAN_HD bool resample_same_phase(unsigned long long up, unsigned long long down, unsigned long long lanes)
{
    return (lanes * down) % up == 0;  // (inside the budget down < 2^28: no overflow)
}

// The lanes of a workgroup that own outputs in the shared-phase instance of the tiled kernel: the largest multiple of
// up / gcd(up, down) within the 256 threads, where that keeps at least three quarters of them busy (256 for up = 1, 2, 4, ..;
// 255 for 3 / 1; none for 160 / 441, whose phases repeat every 160 outputs).  0: no such instance, every thread walks its outputs
// one at a time.  A tile of that instance is four outputs per lane.
KOFFT_PLAN_HD unsigned resample_phase_lanes(unsigned long long up, unsigned long long down)
{
    unsigned long long a = up, b = down;
    while (b) {
        const unsigned long long r = a % b;
        a = b;
        b = r;
    }
    const unsigned long long period = up / a;
    if (period > kResampleThreads) return 0;
    const unsigned lanes = (unsigned)(kResampleThreads / period * period);
    return lanes >= kResampleThreads / 4 * 3 ? lanes : 0;
}

// the outputs of one tile: four per owning lane, kResampleTile at most
KOFFT_PLAN_HD unsigned resample_tile_outputs(unsigned long long up, unsigned long long down)
{
    const unsigned lanes = resample_phase_lanes(up, down);
    return lanes ? 4 * lanes : kResampleTile;
}

}  // namespace host
}  // namespace kofft
