// welch_impl.hip.h -- Welch power spectra and cross spectra of rows: the sums over frames of |X[k]|^2 (or conj(X) Y) of
// the one-sided STFT of every row, in the order include/kofft_hip.h fixes: groups of KOFFT_HIP_WELCH_GROUP frames summed ascending
// from +0, the groups' partials summed ascending from +0, one multiplication by `scale`, (flag) one by 2 on the interior bins.  f32 only.
//
//  * FUSED (win_len 64 .. 4096, a power of two): welch_fused_kernel.  A slot of TPT = n / R threads owns ONE group of one row; it loads
//    and windows frame after frame as StftIO does (x * w inside the row, +0 past its end), transforms it in its LDS exchange slot with
//    fft_wg_kernel's own passes (wg_compute / wg_exchange, unchanged: the spectrum bits are the one-sided STFT's) and adds the product of
//    every bin o <= n/2 it holds into a register -- a thread holds the same bins in every frame.  The cross spectrum runs the two
//    transforms of a frame back to back.  The frames never reach memory.  A row of one group is scaled and stored from here; otherwise
//    the partial goes to the scratch and welch_total_kernel adds the row's partials.
//  * COMPOSED (every other window length, mode 0): the one-sided frames of a chunk of whole groups into the scratch through the existing
//    dispatch, welch_partial_kernel (a lane per group and bin walks its frames), then welch_total_kernel.
//
// welch_total_kernel carries a row's running total across chunks in the caller's output: a chunk that begins inside a row reads what the
// chunk before it left there (un-scaled), and the chunk that holds the row's last group scales.
#pragma once

#include "host_common.hip.h"
#include "welch_cut.h"

namespace kofft {

// one term of the sums, un-fused (the translation unit is built with -ffp-contract=off)
template <bool CSD>
struct WelchAcc;
template <>
struct WelchAcc<false> {
    float s;
    __device__ __forceinline__ void zero() { s = 0.0f; }
    __device__ __forceinline__ void add(cpx<float> x, cpx<float>)
    {
        const float p = x.re * x.re + x.im * x.im;  // StftMagIO::sumsq
        s = s + p;
    }
    __device__ __forceinline__ void store(float *dst, size_t bin, float scale, float twice, bool final) const
    {
        dst[bin] = final ? (s * scale) * twice : s;
    }
};
template <>
struct WelchAcc<true> {
    float re, im;
    __device__ __forceinline__ void zero() { re = 0.0f; im = 0.0f; }
    __device__ __forceinline__ void add(cpx<float> x, cpx<float> y)
    {
        const float cr = x.re * y.re + x.im * y.im;  // conj(X) Y
        const float ci = x.re * y.im - x.im * y.re;
        re = re + cr;
        im = im + ci;
    }
    __device__ __forceinline__ void store(float *dst, size_t bin, float scale, float twice, bool final) const
    {
        dst[2 * bin] = final ? (re * scale) * twice : re;  // 4-byte stores: the output is float-aligned only
        dst[2 * bin + 1] = final ? (im * scale) * twice : im;
    }
};

// Groups [g_first, g_first + g_count) of the flat group index row * ngroups + group; slot s of workgroup b owns group g_first + b * XPB + s.
// final: ngroups == 1, the row's total IS the partial (+0 + p has p's bits: a sum seeded with +0 is never -0): dst = the output, row-major
// rows of K bins.  Otherwise dst = the chunk's partials, group g at dst + (g - g_first) * K (* 2).
template <int L, int RL, int BLOCK, bool CSD>
__global__ __launch_bounds__(BLOCK) void welch_fused_kernel(const StftIO iox, const float *__restrict__ sig_y, const cpx<float> *__restrict__ tw,
                                                            const size_t row_stride, const size_t frames, const size_t ngroups,
                                                            const size_t g_first, const size_t g_count, float *__restrict__ dst,
                                                            const float scale, const int twice, const int final)
{
    constexpr int N = 1 << L, R = 1 << RL, TPT = N / R, XPB = BLOCK / TPT, NP = (L + RL - 1) / RL, H = N / 2;
    static_assert(TPT >= 1 && BLOCK % TPT == 0 && NP >= 2 && NP <= 5, "bad geometry");
    using G0 = WgGeom<L, RL, 0>;
    using GL = WgGeom<L, RL, NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];

    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const size_t gl = (size_t)blockIdx.x * XPB + slot;  // group of this launch
    const bool active = gl < g_count;
    const size_t gi = g_first + (active ? gl : 0), row = gi / ngroups, f0 = (gi - row * ngroups) * host::kWelchGroup;
    const int cnt = !active ? 0 : (frames - f0 < host::kWelchGroup ? (int)(frames - f0) : (int)host::kWelchGroup);
    StftIO io = iox;
    io.signal = iox.signal + row * row_stride;
    const float *__restrict__ ys = CSD ? sig_y + row * row_stride : nullptr;

    float w[R];
#pragma unroll
    for (int u = 0; u < R; ++u) w[u] = io.window[G0::in_index(tau, u)];
    WelchAcc<CSD> acc[R];
#pragma unroll
    for (int u = 0; u < R; ++u) acc[u].zero();

    // one windowed frame into v, transformed: fft_wg_kernel's passes
    auto transform = [&](const float *__restrict__ sig, const size_t start, const int rem, cpx<float> (&v)[R]) {
        if (rem == N) {
#pragma unroll
            for (int u = 0; u < R; ++u) v[u] = io.finish_in(sig[start + G0::in_index(tau, u)], w[u]);
        } else {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int i = G0::in_index(tau, u);
                v[u] = io.finish_rem(i, i < rem ? sig[start + i] : 0.0f, w[u], rem);
            }
        }
        wg_compute<float, L, RL, 0>(v, io, tw, 0, tau);
        if constexpr (NP > 1) { wg_exchange<float, L, RL, 0, false, false, XPB>(v, smem_raw, tau, slot); wg_compute<float, L, RL, 1>(v, io, tw, 0, tau); }
        if constexpr (NP > 2) { wg_exchange<float, L, RL, 1, false, false, XPB>(v, smem_raw, tau, slot); wg_compute<float, L, RL, 2>(v, io, tw, 0, tau); }
        if constexpr (NP > 3) { wg_exchange<float, L, RL, 2, false, false, XPB>(v, smem_raw, tau, slot); wg_compute<float, L, RL, 3>(v, io, tw, 0, tau); }
        if constexpr (NP > 4) { wg_exchange<float, L, RL, 3, false, false, XPB>(v, smem_raw, tau, slot); wg_compute<float, L, RL, 4>(v, io, tw, 0, tau); }
    };

    for (int j = 0; j < (int)host::kWelchGroup; ++j) {  // (every slot of the workgroup walks all rounds: the exchanges synchronise the workgroup)
        const bool live = j < cnt;
        const size_t f = f0 + (live ? j : 0);
        const int rem = live ? io.frame_rem(f) : 0;  // a slot without a frame transforms zeros and adds nothing
        const size_t start = rem ? f * io.hop : 0;
        cpx<float> x[R], y[R];
        if (j > 0) __syncthreads();  // the gathers of the transform before this one are done
        transform(io.signal, start, rem, x);
        if constexpr (CSD) {
            __syncthreads();
            transform(ys, start, rem, y);
        }
        if (live) {
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (GL::out_index(tau, u) <= H) acc[u].add(x[u], CSD ? y[u] : x[u]);
        }
    }
    if (!active) return;
    constexpr size_t K = H + 1;
    float *out = dst + (final ? gi : gl) * K * (CSD ? 2 : 1);
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int o = GL::out_index(tau, u);
        if (o <= H) acc[u].store(out, (size_t)o, scale, (twice && o >= 1 && o < H) ? 2.0f : 1.0f, final != 0);
    }
}

namespace host {

// The composed route's partials: frames of nt consecutive flat indices from t0 (a chunk of whole groups) lie at spec_x (spec_y) with
// `fstride` complex values per frame, bins k < K first.  A lane per (group of the chunk, bin): part[(g - g_first) * K + k] (CSD: re, im).
template <bool CSD>
static __global__ __launch_bounds__(256) void welch_partial_kernel(const cpx<float> *__restrict__ spec_x, const cpx<float> *__restrict__ spec_y,
                                                                   float *__restrict__ part, const size_t fstride, const size_t K,
                                                                   const size_t frames, const size_t ngroups, const size_t t0,
                                                                   const size_t g_first, const size_t total /* groups of the chunk * K */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t gl = idx / K, k = idx - gl * K, gi = g_first + gl, row = gi / ngroups, f0 = (gi - row * ngroups) * kWelchGroup;
    const size_t cnt = frames - f0 < kWelchGroup ? frames - f0 : kWelchGroup;
    const size_t at = (row * frames + f0 - t0) * fstride + k;
    WelchAcc<CSD> acc;
    acc.zero();
    for (size_t j = 0; j < cnt; ++j) {
        const cpx<float> x = spec_x[at + j * fstride];
        acc.add(x, CSD ? spec_y[at + j * fstride] : x);
    }
    acc.store(part, idx, 1.0f, 1.0f, false);
}

// The rows' totals from the partials of groups [g_first, g_first + g_count): a lane per (row the chunk touches, value e of its K * (CSD ? 2 : 1)
// floats) adds its row's partials ascending onto +0, or onto the running total the earlier chunks left in `out` when the chunk begins
// inside the row; the row's last group scales: (t * scale) (* 2 on bins 1 <= k < k_hi).
static __global__ __launch_bounds__(256) void welch_total_kernel(const float *__restrict__ part, float *__restrict__ out, const size_t vals,
                                                                 const int per_bin, const size_t ngroups, const size_t g_first,
                                                                 const size_t g_count, const float scale, const int twice, const size_t k_hi,
                                                                 const size_t total /* rows of the chunk * vals */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t row0 = g_first / ngroups, rl = idx / vals, e = idx - rl * vals, row = row0 + rl;
    const size_t row_g = row * ngroups, g_end = g_first + g_count;
    const size_t ga = row_g > g_first ? row_g : g_first, gb = row_g + ngroups < g_end ? row_g + ngroups : g_end;
    float *o = out + row * vals + e;
    float t = ga == row_g ? 0.0f : *o;
    const float *p = part + (ga - g_first) * vals + e;
    size_t n = gb - ga;
    for (; n >= 8; n -= 8, p += 8 * vals) {  // eight loads in flight, the adds in order
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) q[i] = p[(size_t)i * vals];
#pragma unroll
        for (int i = 0; i < 8; ++i) t = t + q[i];
    }
    for (; n > 0; --n, p += vals) t = t + *p;
    if (gb == row_g + ngroups) {
        const size_t k = e / (size_t)per_bin;
        t = t * scale;
        if (twice && k >= 1 && k < k_hi) t = t * 2.0f;
    }
    *o = t;
}

}  // namespace host
}  // namespace kofft
