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
// convolve_filter_kernel with complex and conjugated taps: element e is point e & (block - 1) of filter e >> lb.
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

// convolve_gather_kernel for filter f of the bank: y holds ifft's results (conj and scale applied)
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
// convolve_fused_kernel<L>'s geometry, item walk and per-lane row bounds.  The first transform's bins stay in 2 R registers (X) while
// the loop over the filters multiplies, reorders through the item's exchange slot, transforms and stores: no second LDS slot, and the
// 4096-point instance keeps its two waves per SIMD (the resource table).
template <int L, class Kind>
__global__ __launch_bounds__(256) void convolve_bank_fused_kernel(const float *__restrict__ x, const cpx<float> *__restrict__ H,
                                                                  typename Kind::Out *__restrict__ out, const cpx<float> *__restrict__ tw,
                                                                  const ConvShape s, const size_t filters, const float scale)
{
    using Geo = HilbertGeom<L>;
    constexpr int N = Geo::N, R = Geo::R, TPT = Geo::TPT, XPB = Geo::XPB;
    using G0 = WgGeom<L, Geo::RL, 0>;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const size_t item = (size_t)blockIdx.x * XPB + slot;
    const bool live = item < s.items;  // (the last workgroup's spare slots: zeros in, nothing out)
    const size_t it = live ? item : 0;
    const size_t row = s.row_of(it), b = s.b0 + (it - row * s.nbw);
    const long long first = (long long)(b * s.hop) - (long long)(s.nh - 1);  // the sample index of frame element 0
    cpx<float> X[R];
    {
        // elements [lo, hi) of the frame are samples of this row (convolve_fused_kernel): no lane reads outside its row
        const int lo = first < 0 ? (int)-first : 0;
        const long long left = (long long)s.nx - first;
        const int hi = !live || left <= 0 ? 0 : (left < (long long)N ? (int)left : N);
        const float *xr = x + row * s.nx + first;
        float raw[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int i = G0::in_index(0, u) + tau;
            raw[u] = (i >= lo && i < hi) ? xr[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) X[u] = mk<float>(raw[u], 0.0f);
    }
    hilbert_forward<L>(X, smem_raw, tw, tau, slot);
    // Element k of y_f goes to full_out[b * hop + k - (nh - 1)] for k >= nh - 1; kept where that lies inside the window: k in [klo, khi)
    const long long shift = (long long)(b * s.hop) - (long long)(s.nh - 1) - (long long)s.out_first;  // window index = k + shift
    const long long lo64 = -shift > (long long)(s.nh - 1) ? -shift : (long long)(s.nh - 1);
    const long long hi64 = (long long)s.out_len - shift;
    const int klo = lo64 < (long long)N ? (int)lo64 : N;
    const int khi = !live || hi64 <= 0 ? 0 : (hi64 < (long long)N ? (int)hi64 : N);
    cpx<float> *buf = reinterpret_cast<cpx<float> *>(smem_raw) + (size_t)slot * lds_elems(N);
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
        // last pass's output order -> pass 0's input order, through the item's exchange slot
        __syncthreads();  // every gather of the previous transform's last exchange is done
#pragma unroll
        for (int u = 0; u < R; ++u) buf[lds_pad(GL::out_index(tau, u))] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = buf[lds_pad(G0::in_index(tau, u))];
        __syncthreads();  // (the second transform's first exchange scatters into the same cells)
        hilbert_forward<L>(v, smem_raw, tw, tau, slot);
        // ifft's last conj and * scale (fft.rs:1168-1172)
        typename Kind::Out *orow = out + ((row * filters + f) * s.out_len + shift);
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int k = GL::out_index(0, u) + tau;
            if (k >= klo && k < khi) st_stream(orow + k, Kind::of(v[u].re * scale, (-v[u].im) * scale));
        }
    }
}

template <int L, class Kind>
int launch_convolve_bank_fused(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, void *d_out, const cpx<float> *tw,
                               const ConvShape &s, size_t filters)
{
    using Geo = HilbertGeom<L>;
    constexpr size_t lds = Geo::lds_bytes();
    static_assert(lds <= 64 * 1024, "LDS budget");
    const size_t blocks = (s.items + Geo::XPB - 1) / Geo::XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    const float scale = 1.0f / (float)Geo::N;  // fft.rs:1167
    hipLaunchKernelGGL((convolve_bank_fused_kernel<L, Kind>), dim3((unsigned)blocks), dim3(Geo::BLOCK), lds, ctx->stream, d_x, H,
                       static_cast<typename Kind::Out *>(d_out), tw, s, filters, scale);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft
