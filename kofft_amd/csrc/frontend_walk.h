// frontend_walk.h -- one filter of cepstrum::mel_filterbank (cepstrum.rs:52-70) over the plan of kofft_tables::mel_plan_build, for a
// lane that owns ONE (frame, filter) pair instead of a whole row (mfcc_impl.hip.h's sweep).  Shared by the fused front-end kernel
// (frontend_impl.hip.h) and the host program that compares it with the reference's two loops (tests/cpp/sanitize_frontend_walk.cpp).
//
// plan = [seg: 2 (num_mel + 1) ints | live: num_mel ints], w = 2 n_fft floats: segment s is [seg[2 s], seg[2 s + 1]), the edges
// [bins[s], bins[s + 1]) clamped to the row; w[2 k] is the rise weight of the segment that holds k (filter s), w[2 k + 1] its fall
// weight (filter s - 1).  Filter m adds its rise terms over segment m, then its fall terms over segment m + 1, ascending k, from a
// +0 seed, one multiply and one add per term (the translation unit is built with -ffp-contract=off): the reference's order, so the
// sum has the reference's bits.  A dead filter (an empty rise or fall before clamping) is +0, whatever it summed.
#pragma once

#if defined(__HIPCC__)
#define KOFFT_WALK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KOFFT_WALK_HD inline
#endif

namespace kofft {

KOFFT_WALK_HD float frontend_filter_walk(const int *plan, const float *w, const float *x, const int num_mel, const int m)
{
    const int *seg = plan, *live = plan + 2 * (num_mel + 1);
    float acc = 0.0f;
    for (int k = seg[2 * m], e = seg[2 * m + 1]; k < e; ++k) {
        const float t = w[2 * k] * x[k];  // cepstrum.rs:59
        acc = acc + t;
    }
    for (int k = seg[2 * m + 2], e = seg[2 * m + 3]; k < e; ++k) {
        const float t = w[2 * k + 1] * x[k];  // cepstrum.rs:64
        acc = acc + t;
    }
    return live[m] ? acc : 0.0f;
}

}  // namespace kofft
