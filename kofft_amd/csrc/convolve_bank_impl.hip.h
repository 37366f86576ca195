// convolve_bank_impl.hip.h -- overlap-save FFT convolution / correlation of rows of f32 samples with a bank of `filters` filters that
// all rows share.  The definition is convolve_impl.hip.h's with a filter index:
//   H_f      = fft((re, im) of tap i of filter f, zero-padded to block); real taps: (h[f][i], +0); complex taps: interleaved (re, im)
//              pairs; correlate: the taps reversed, complex ones conjugated as well, conj(h[f][nh - 1 - i])
//   X        = fft(frame), the frame of convolve_impl.hip.h -- ONCE per (row, block)
//   Y_f[k]   = X[k] * H_f[k], Complex::mul un-fused (num.rs:162-165)
//   y_f      = ifft(Y_f) (fft.rs:1134-1174: conj, fft, conj, * 1 / block): re = v.re * scale, im = (-v.im) * scale
//   full_out[row][f][b * hop + j] = kind(y_f[nh - 1 + j]), j < hop;  kind: the real part, the (re, im) pair, or the magnitude
//              sqrtf(re * re + im * im) of the scaled values (the sum un-fused, the root correctly rounded)
// and the caller receives full_out[out_first .. out_first + out_len) of every (row, filter), dense [rows][filters][out_len].  F filters
// cost F + 1 transforms per frame where F calls of the one-filter entry cost 2 F, and the signal is read once.  Two routes, the same
// operations per element, over the same flat items (ConvShape) as the one-filter family:
//  * fused (block = 32 .. 4096, a 4-byte aligned input, kofft_hip_set_convolve_bank_fused on): convolve_bank_fused_kernel<L, Kind>,
//    convolve_fused_kernel<L> with the first transform's bins kept in registers and a loop over the filters behind it;
//  * composed (every other block up to 65536, unaligned inputs, the switch off): convolve_expand_kernel and fft_dev once per chunk of
//    items, then per filter convolve_bank_mul_kernel into a second buffer, fft_dev(inverse) and convolve_bank_gather_kernel<Kind>.
// The filter spectra are computed first on every call: convolve_bank_filter_kernel, then fft_dev in place, at the head of the scratch.
// The filter and gather kernels serve the one-filter family as well.
// x / h and out must not overlap.
#pragma once

#include "convolve_impl.hip.h"

namespace kofft {
namespace host {

constexpr unsigned kBankCorrelate = 1u, kBankComplexTaps = 2u, kBankKindShift = 2u, kBankKindMask = 3u;

// ---- output kinds: flag bits 2-3 ------------------------------------------------------------------------------------------------
// of(re, im): the stored element from the scaled parts of y_f
struct BankReal {
    using Out = float;
    __device__ __forceinline__ static Out of(float re, float) { return re; }
};
struct BankComplex {
    using Out = cpx<float>;
    __device__ __forceinline__ static Out of(float re, float im) { return mk<float>(re, im); }
};
struct BankMagnitude {
    using Out = float;
    // sqrtf is correctly rounded here (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), as StftMagIO's (fft_wg.hip.h)
    __device__ __forceinline__ static Out of(float re, float im) { return sqrtf(re * re + im * im); }
};

// ---- filter spectra -------------------------------------------------------------------------------------------------------------
// Element e is point e & (block - 1) of filter e >> lb: real or complex taps, reversed (complex ones conjugated as well) to correlate.
// The one-filter family's spectra too (k_convolve_f32.hip: filter_spectra), with real taps and one filter per row or one in all.
__global__ __launch_bounds__(256) void convolve_bank_filter_kernel(const float *__restrict__ h, cpx<float> *__restrict__ H, const size_t nh,
                                                                   const int lb, const unsigned flags, const size_t total)
{
    const size_t mask = (size_t(1) << lb) - 1;
    const bool reverse = flags & kBankCorrelate, cplx = flags & kBankComplexTaps;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t f = e >> lb, i = e & mask;
        cpx<float> v = mk<float>(0.0f, 0.0f);
        if (i < nh) {
            const size_t at = f * nh + (reverse ? nh - 1 - i : i);
            if (cplx) {
                const float im = h[2 * at + 1];
                v = mk<float>(h[2 * at], reverse ? -im : im);
            } else {
                v = mk<float>(h[at], 0.0f);
            }
        }
        H[e] = v;
    }
}

// ---- composed route -------------------------------------------------------------------------------------------------------------
// y = X * H_f over a chunk of transformed frames, into the second buffer (X stays for the next filter)
__global__ __launch_bounds__(256) void convolve_bank_mul_kernel(const cpx<float> *__restrict__ X, const cpx<float> *__restrict__ Hf,
                                                                cpx<float> *__restrict__ y, const int lb, const size_t total)
{
    const size_t mask = (size_t(1) << lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256)
        st_stream(y + e, cmul(X[e], Hf[e & mask]));  // num.rs:162-165
}

// The kept part of every frame of a chunk into the window of (row, filter f): y holds ifft's results (conj and scale applied).  The
// one-filter family's gather too: BankReal with filters = 1, f = 0 addresses out + row * out_len.
template <class Kind>
__global__ __launch_bounds__(256) void convolve_bank_gather_kernel(const cpx<float> *__restrict__ y, typename Kind::Out *__restrict__ out,
                                                                   const ConvShape s, const size_t filters, const size_t f,
                                                                   const size_t item0, const size_t total)
{
    const size_t mask = (size_t(1) << s.lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t it = item0 + (e >> s.lb), i = e & mask;
        if (i < s.nh - 1) continue;
        const size_t row = s.row_of(it), b = s.b0 + (it - row * s.nbw);
        const size_t pos = b * s.hop + (i - (s.nh - 1));
        if (pos >= s.out_first && pos - s.out_first < s.out_len) {
            const cpx<float> v = y[e];
            st_stream(out + (row * filters + f) * s.out_len + (pos - s.out_first), Kind::of(v.re, v.im));
        }
    }
}

// ---- fused route: block = 2^L, L = 5 .. 12 --------------------------------------------------------------------------------------
// convolve_fused_kernel<L>'s geometry, item walk and per-lane row bounds (conv_item, conv_load_frame, conv_window).  The first
// transform's bins stay in 2 R registers (X) while the loop over the filters multiplies, reorders through the item's exchange slot,
// transforms and stores: no second LDS slot, and the 4096-point instance keeps its two waves per SIMD (the resource
// table).
template <int L, class Kind>
__global__ __launch_bounds__(256) void convolve_bank_fused_kernel(const float *__restrict__ x, const cpx<float> *__restrict__ H,
                                                                  typename Kind::Out *__restrict__ out, const cpx<float> *__restrict__ tw,
                                                                  const ConvShape s, const size_t filters, const float scale)
{
    using Geo = FusedGeom<L>;
    constexpr int N = Geo::N, R = Geo::R, TPT = Geo::TPT;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const ConvItem c = conv_item<L>(s, slot);
    cpx<float> X[R];
    conv_load_frame<L>(X, x, s, c, tau);
    fused_forward<L>(X, smem_raw, tw, tau, slot);
    const ConvWindow w = conv_window<N>(s, c);
    for (size_t f = 0; f < filters; ++f) {  // (uniform over the workgroup: every barrier below is met by all of it)
        cpx<float> v[R];
        {   // Y = X * H_f (num.rs:162-165), then ifft's conj (fft.rs:1163-1165)
            const cpx<float> *Hr = H + f * (size_t)N + tau;
            cpx<float> hv[R];
#pragma unroll
            for (int u = 0; u < R; ++u) hv[u] = Hr[GL::out_index(0, u)];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const cpx<float> y = cmul(X[u], hv[u]);
                v[u] = mk<float>(y.re, -y.im);
            }
        }
        fused_reorder<L>(v, smem_raw, tau, slot);
        fused_forward<L>(v, smem_raw, tw, tau, slot);
        // ifft's last conj and * scale (fft.rs:1168-1172)
        typename Kind::Out *orow = out + ((c.row * filters + f) * s.out_len + w.shift);
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int k = GL::out_index(0, u) + tau;
            if (k >= w.klo && k < w.khi) st_stream(orow + k, Kind::of(v[u].re * scale, (-v[u].im) * scale));
        }
    }
}

}  // namespace host
}  // namespace kofft
