// pfb_impl.hip.h -- the polyphase filter bank of rows of f32: a prototype filter of T M taps folded onto an M-point transform
// (analysis, a weighted-overlap-add channelizer) and the inverse transforms overlap-added under a synthesis filter.
// The reference has no such entry point; every value is a composition of its operations, as include/kofft_hip.h states them.
//
// Analysis, item t = row * frames + f, nh = T M taps h, hop D, `lead` virtual zeros in front of every row:
//   g_t  = h[j + tM] * x[fD + j + tM - lead]   where that sample exists in its own row, +0 elsewhere
//   u[j] = (..((g_0 + g_1) + g_2)..) + g_{T-1}  one accumulator started by g_0
//   Z    = fft((u[j], +0))                      (fft.rs:1054-1132; nothing for M == 1);  bins k < `bins` of Z are stored
// Two routes, the same operations per element:
//  * fused (M = 32 .. 4096, 4-byte aligned x and h; the default up to M = 1024, kofft_hip_set_pfb_fused(ctx, 2) beyond):
//    pfb_fused_kernel<L, IO>, one pass over HBM on the
//    shared register transform (FusedGeom, fused_forward; fused_rows.hip.h).  Items of one workgroup are neighbouring frames, whose
//    overlapping samples the caches serve; they may belong to different rows of signals, so every sample is tested against its own
//    row's bounds (plain loads, no shared descriptor);
//  * composed (every other M, unaligned inputs, the switch at 0): pfb_fold_kernel into the context's scratch, fft_dev, and
//    pfb_prefix_kernel where bins < M, in chunks of flat items.
// Synthesis: the inverse transforms of a chunk of frames go into scratch as M reals per frame -- pfb_inverse_fused_kernel<L>, or
// pfb_complete_kernel, inverse fft_dev and pfb_real_kernel --, then pfb_ola_kernel: one thread per output sample, its covering frames
// in ascending order.
#pragma once

#include "frame_cut.h"
#include "fused_rows.hip.h"

namespace kofft {
namespace host {

// ---- the analysis IO policy: item(t) is computed once per thread (or element), fold(it, j) is u[j] of that item ---------------------
// No lane reads a sample of another row.
struct PfbIO {
    const float *x, *h;
    cpx<float> *out;
    size_t m, taps, nx, row_stride, frames, hop, lead, bins;
    struct Item {
        const float *xr;
        long long first;  // the sample index of tap 0
    };
    __device__ __forceinline__ Item item(size_t t) const
    {
        const size_t row = t / frames, f = t - row * frames;
        return Item{x + row * row_stride, (long long)(f * hop) - (long long)lead};
    }
    // tap i of the item: one product, or +0 where the sample does not exist
    __device__ __forceinline__ float term(const Item &it, size_t i) const
    {
        const long long s = it.first + (long long)i;
        return (s >= 0 && s < (long long)nx) ? h[i] * it.xr[s] : 0.0f;
    }
    __device__ __forceinline__ float fold(const Item &it, size_t j) const
    {
        float acc = term(it, j);
        for (size_t t = 1; t < taps; ++t) acc = acc + term(it, j + t * m);
        return acc;
    }
};

// ---- composed analysis: flat grid-stride kernels, element e of a chunk is point e % M of item item0 + e / M -------------------------
template <class IO>
__global__ __launch_bounds__(256) void pfb_fold_kernel(const IO io, cpx<float> *__restrict__ z, const size_t item0, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t q = e / io.m, j = e - q * io.m;
        const typename IO::Item it = io.item(item0 + q);
        st_stream(z + e, mk<float>(io.fold(it, j), 0.0f));
    }
}

// dst[q][k] = src[q][k] for k < bins: the kept bins of every transform of a chunk
static __global__ __launch_bounds__(256) void pfb_prefix_kernel(const cpx<float> *__restrict__ src, cpx<float> *__restrict__ dst, const size_t m,
                                                               const size_t bins, const size_t total /* transforms * bins */)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t q = e / bins, k = e - q * bins;
        st_stream(dst + e, src[q * m + k]);
    }
}

// ---- fused analysis: M = 2^L, L = 5 .. 12 --------------------------------------------------------------------------------------------
// FusedGeom<L>::XPB items per 256-thread workgroup, TPT threads each.  Pass 0's register u of thread tau holds element e =
// in_index(0, u) + tau of u[]: R accumulators per thread over a run-time loop on the taps t, and for a fixed (u, t) the loads of x and
// h are consecutive over tau.  After the transform register u holds bin k = out_index(0, u) | tau, stored where k < bins.  A spare
// slot of the last workgroup transforms zeros and stores nothing.  (The last parameter is launch_fused_items' 1 / M, which the
// forward transform does not use.)
template <int L, class IO>
__global__ __launch_bounds__(256) void pfb_fused_kernel(const IO io, const cpx<float> *__restrict__ tw, const size_t items, const float)
{
    using Geo = FusedGeom<L>;
    constexpr int M = Geo::N, R = Geo::R, TPT = Geo::TPT, XPB = Geo::XPB;
    using G0 = WgGeom<L, Geo::RL, 0>;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const size_t t = (size_t)blockIdx.x * XPB + slot;
    const bool live = t < items;
    cpx<float> v[R];
    {
        const typename IO::Item it = io.item(live ? t : 0);
        const size_t taps = live ? io.taps : 0;
        float acc[R];
#pragma unroll
        for (int u = 0; u < R; ++u) acc[u] = live ? io.term(it, (size_t)(G0::in_index(0, u) + tau)) : 0.0f;
        for (size_t k = 1; k < taps; ++k) {
            const size_t base = k * (size_t)M + (size_t)tau;
            float g[R];
#pragma unroll
            for (int u = 0; u < R; ++u) g[u] = io.term(it, base + (size_t)G0::in_index(0, u));
#pragma unroll
            for (int u = 0; u < R; ++u) acc[u] = acc[u] + g[u];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = mk<float>(acc[u], 0.0f);
    }
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    if (!live) return;
    cpx<float> *orow = io.out + t * io.bins;
    const size_t bins = io.bins;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const size_t k = (size_t)(GL::out_index(0, u) + tau);
        if (k < bins) st_stream(orow + k, v[u]);
    }
}

// ---- synthesis: the inverse transforms of a chunk of frames, M reals per frame ------------------------------------------------------
// Bin k of the frame ifft sees: the frame's own bin, or for k >= bins (the one-sided form, bins = M/2 + 1) F[k] = (half[M-k].re,
// -half[M-k].im).  The imaginary parts of bins 0 and M/2 are used as given.
__device__ __forceinline__ cpx<float> pfb_bin(const cpx<float> *frame, const size_t m, const size_t bins, const size_t k)
{
    if (k < bins) return frame[k];
    const cpx<float> c = frame[m - k];
    return mk<float>(c.re, -c.im);
}

// composed: full[q][k] = F[k] of frame q of the chunk, for the inverse fft_dev
static __global__ __launch_bounds__(256) void pfb_complete_kernel(const cpx<float> *__restrict__ spec, cpx<float> *__restrict__ full, const size_t m,
                                                                 const size_t bins, const size_t total /* transforms * m */)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t q = e / m, k = e - q * m;
        st_stream(full + e, pfb_bin(spec + q * bins, m, bins, k));
    }
}

static __global__ __launch_bounds__(256) void pfb_real_kernel(const cpx<float> *__restrict__ z, float *__restrict__ v, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) st_stream(v + e, z[e].re);
}

// fused: completion and conj on the loads, the forward transform, re * 1 / M (fft.rs:1168-1172; the conj on the way out leaves re
// alone) stored contiguously over tau.  spec: `items` frames of `bins` complex; v: `items` rows of M reals.
template <int L>
__global__ __launch_bounds__(256) void pfb_inverse_fused_kernel(const cpx<float> *__restrict__ spec, float *__restrict__ vout, const size_t bins,
                                                                const cpx<float> *__restrict__ tw, const size_t items, const float scale)
{
    using Geo = FusedGeom<L>;
    constexpr int M = Geo::N, R = Geo::R, TPT = Geo::TPT, XPB = Geo::XPB;
    using G0 = WgGeom<L, Geo::RL, 0>;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const size_t t = (size_t)blockIdx.x * XPB + slot;
    const bool live = t < items;
    cpx<float> v[R];
    {
        const cpx<float> *frame = spec + (live ? t : 0) * bins;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const cpx<float> c = live ? pfb_bin(frame, (size_t)M, bins, (size_t)(G0::in_index(0, u) + tau)) : mk<float>(0.0f, 0.0f);
            v[u] = mk<float>(c.re, -c.im);  // ifft's conj on the way in (fft.rs:1163-1165)
        }
    }
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    if (!live) return;
    float *orow = vout + t * (size_t)M;
#pragma unroll
    for (int u = 0; u < R; ++u) st_stream(orow + GL::out_index(0, u) + tau, v[u].re * scale);
}

// ---- synthesis: overlap-add ------------------------------------------------------------------------------------------------------------
// One piece of a chunk (frame_cut.h): the frames [f0, ...) of rows [row, row + nr) lie dense at v, M reals each, frame f0 of row `row`
// first, a row's frames `frames` apart when nr > 1 (then f0 == 0); where f0 > 0 the frames before f0 that a sample of the piece needs
// lie right before v.  One thread per sample p in [lo, hi) of each row's `full`:
//   full[p] = (sum over f ascending with 0 <= p - fD < nh of g[p - fD] * r_f[(p - fD) mod M]) * scale, the first term starting the
//   accumulator; +0 where no frame covers p,
// stored at out[(row + r) * out_len + p - out_first].
static __global__ __launch_bounds__(256) void pfb_ola_kernel(const float *__restrict__ v, const float *__restrict__ g, float *__restrict__ out,
                                                            const size_t m, const size_t nh, const size_t hop, const size_t frames, const size_t row,
                                                            const size_t f0, const size_t lo, const size_t hi, const size_t out_first,
                                                            const size_t out_len, const float scale, const size_t total)
{
    const size_t span = hi - lo;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / span, p = lo + (e - r * span);
        const size_t flo = p >= nh ? (p - nh) / hop + 1 : 0;
        size_t fhi = p / hop;
        if (fhi > frames - 1) fhi = frames - 1;
        float res = 0.0f;
        if (flo <= fhi) {
            // frame f of row `row + r` (f < f0: one of the frames before the piece)
            const float *vr = v + ((long long)(r * frames) - (long long)f0) * (long long)m;
            size_t i = p - flo * hop;
            float acc = g[i] * vr[flo * m + i % m];
            for (size_t f = flo + 1; f <= fhi; ++f) {
                i -= hop;
                acc = acc + g[i] * vr[f * m + i % m];
            }
            res = acc * scale;
        }
        st_stream(out + (row + r) * out_len + (p - out_first), res);
    }
}

}  // namespace host
}  // namespace kofft
