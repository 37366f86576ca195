// convolve_impl.hip.h -- overlap-save FFT convolution / correlation of rows of f32 samples with f32 taps on device pointers (DESIGN.md
// 5.25).  The reference has no such entry point; every value is a composition of its operations.
//
// rows signals of nx samples, a filter of nh taps (one for all rows or one per row), a power-of-two block >= nh, hop = block - nh + 1,
// full = nx + nh - 1, nb = ceil(full / hop) blocks per row:
//   H        = fft((h[i], +0) zero-padded to block)            (fft.rs:1054-1132; correlate: the taps reversed, h[nh - 1 - i])
//   frame[i] = (x[b * hop - (nh - 1) + i], +0) where that sample exists, (+0, +0) elsewhere;  X = fft(frame)
//   Y[k]     = X[k] * H[k], Complex::mul un-fused (num.rs:162-165)
//   y        = ifft(Y)                                           (fft.rs:1134-1174: conj, fft, conj, * 1 / block)
//   full_out[b * hop + j] = y[nh - 1 + j].re, j < hop
// and the caller receives full_out[out_first .. out_first + out_len) of every row, dense.  Blocks wholly outside that window are not
// computed: the routes walk flat items = row * nbw + (b - b0) over the nbw blocks b0 .. b0 + nbw - 1 that touch it.  Two routes, the
// same operations per element:
//  * fused (block = 32 .. 4096, a 4-byte aligned input, kofft_hip_set_convolve_fused on): convolve_fused_kernel<L>, one pass over
//    HBM, on the shared two-transform machinery (FusedGeom, fused_forward, fused_reorder; fused_rows.hip.h).  It keeps its own
//    body: items of one workgroup may belong to different rows, so every lane tests its own sample against its own row's bounds
//    (plain loads, no shared descriptor), and the store keeps a part of each frame only;
//  * composed (every other block up to 65536, unaligned inputs, the switch off): convolve_expand_kernel into the context's scratch,
//    fft_dev, convolve_mul_kernel, fft_dev(inverse), convolve_bank_gather_kernel<BankReal> (the bank's, with one filter), in chunks
//    of flat items (a seam may fall inside a row).
// The filter spectra are computed first on every call: convolve_bank_filter_kernel (the bank's, with real taps), then fft_dev in
// place, at the head of the scratch.
// x / h and out must not overlap.
#pragma once

#include "fused_rows.hip.h"

namespace kofft {
namespace host {

constexpr size_t kConvolveMaxBlock = size_t(1) << 16;

// One call's shape, by value to every kernel.  Item `it` is block b0 + it % nbw of row it / nbw.
struct ConvShape {
    size_t nx, nh, hop, nbw, b0, out_first, out_len, items;
    int lb;       // log2 block
    int per_row;  // filters == rows (and rows > 1)
    unsigned nbw32;  // nbw when every item index fits 31 bits (a 32-bit division per item), else 0
    __device__ __forceinline__ size_t row_of(size_t it) const { return nbw32 ? (size_t)((unsigned)it / nbw32) : it / nbw; }
};

// ---- composed route ----------------------------------------------------------------------------------------------------------------
// Flat grid-stride kernels as the Hilbert composed route's: element e of a chunk is point e & (block - 1) of item e >> lb.
__global__ __launch_bounds__(256) void convolve_expand_kernel(const float *__restrict__ x, cpx<float> *__restrict__ z, const ConvShape s,
                                                              const size_t item0, const size_t total)
{
    const size_t mask = (size_t(1) << s.lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t it = item0 + (e >> s.lb), i = e & mask;
        const size_t row = s.row_of(it), b = s.b0 + (it - row * s.nbw);
        const size_t at = b * s.hop + i;  // the sample's index + (nh - 1)
        float v = 0.0f;
        if (at >= s.nh - 1 && at - (s.nh - 1) < s.nx) v = x[row * s.nx + (at - (s.nh - 1))];
        st_stream(z + e, mk<float>(v, 0.0f));
    }
}

__global__ __launch_bounds__(256) void convolve_mul_kernel(cpx<float> *__restrict__ z, const cpx<float> *__restrict__ H, const ConvShape s,
                                                           const size_t item0, const size_t total)
{
    const size_t mask = (size_t(1) << s.lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t i = e & mask;
        const size_t f = s.per_row ? s.row_of(item0 + (e >> s.lb)) : 0;
        z[e] = cmul(z[e], H[(f << s.lb) | i]);  // num.rs:162-165
    }
}

// ---- fused route: block = 2^L, L = 5 .. 12 --------------------------------------------------------------------------------------
// FusedGeom<L>::XPB items per 256-thread workgroup, TPT threads each.  Pass 0's register u of thread tau holds element
// in_index(0, u) + tau of its item's frame; after each transform register u holds bin out_index(0, u) | tau.  The three helpers below
// are the item walk and the per-lane bounds of this kernel and of convolve_bank_fused_kernel (convolve_bank_impl.hip.h).

// The item of a thread's slot.  live == false: a spare slot of the last workgroup, zeros in, nothing out (it computes on item 0's row).
struct ConvItem {
    size_t row, b;
    long long first;  // the sample index of frame element 0
    bool live;
};

template <int L>
__device__ __forceinline__ ConvItem conv_item(const ConvShape &s, const int slot)
{
    ConvItem c;
    const size_t item = (size_t)blockIdx.x * FusedGeom<L>::XPB + slot;
    c.live = item < s.items;
    const size_t it = c.live ? item : 0;
    c.row = s.row_of(it);
    c.b = s.b0 + (it - c.row * s.nbw);
    c.first = (long long)(c.b * s.hop) - (long long)(s.nh - 1);
    return c;
}

// The item's frame as (x, +0) in pass-0 input order.  Elements [lo, hi) of the frame are samples of this row: block 0's leading
// zeros and the zeros past nx come from the test, no lane reads outside its row (plain loads: the items of one workgroup may belong to
// different rows, so there is no shared descriptor).
template <int L>
__device__ __forceinline__ void conv_load_frame(cpx<float> *v, const float *x, const ConvShape &s, const ConvItem &c, const int tau)
{
    using Geo = FusedGeom<L>;
    constexpr int N = Geo::N, R = Geo::R;
    using G0 = WgGeom<L, Geo::RL, 0>;
    const int lo = c.first < 0 ? (int)-c.first : 0;
    const long long left = (long long)s.nx - c.first;
    const int hi = !c.live || left <= 0 ? 0 : (left < (long long)N ? (int)left : N);
    const float *xr = x + c.row * s.nx + c.first;
    float raw[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int i = G0::in_index(0, u) + tau;
        raw[u] = (i >= lo && i < hi) ? xr[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < R; ++u) v[u] = mk<float>(raw[u], 0.0f);
}

// Element k of y goes to full_out[b * hop + k - (nh - 1)] for k >= nh - 1; kept where that lies inside the row's window: k in
// [klo, khi), at window index k + shift.
struct ConvWindow {
    long long shift;
    int klo, khi;
};

template <int N>
__device__ __forceinline__ ConvWindow conv_window(const ConvShape &s, const ConvItem &c)
{
    ConvWindow w;
    w.shift = (long long)(c.b * s.hop) - (long long)(s.nh - 1) - (long long)s.out_first;
    const long long lo64 = -w.shift > (long long)(s.nh - 1) ? -w.shift : (long long)(s.nh - 1);
    const long long hi64 = (long long)s.out_len - w.shift;
    w.klo = lo64 < (long long)N ? (int)lo64 : N;
    w.khi = !c.live || hi64 <= 0 ? 0 : (hi64 < (long long)N ? (int)hi64 : N);
    return w;
}

template <int L>
__global__ __launch_bounds__(256) void convolve_fused_kernel(const float *__restrict__ x, const cpx<float> *__restrict__ H, float *__restrict__ out,
                                                             const cpx<float> *__restrict__ tw, const ConvShape s, const float scale)
{
    using Geo = FusedGeom<L>;
    constexpr int N = Geo::N, R = Geo::R, TPT = Geo::TPT;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const ConvItem c = conv_item<L>(s, slot);
    cpx<float> v[R];
    conv_load_frame<L>(v, x, s, c, tau);
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    {   // Y = X * H (num.rs:162-165), then ifft's conj (fft.rs:1163-1165)
        const cpx<float> *Hr = H + (s.per_row ? c.row : 0) * (size_t)N + tau;
        cpx<float> hv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) hv[u] = Hr[GL::out_index(0, u)];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const cpx<float> y = cmul(v[u], hv[u]);
            v[u] = mk<float>(y.re, -y.im);
        }
    }
    fused_reorder<L>(v, smem_raw, tau, slot);
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    // ifft's last conj leaves the real part alone; * scale (fft.rs:1168-1172)
    const ConvWindow w = conv_window<N>(s, c);
    float *orow = out + c.row * s.out_len + w.shift;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int k = GL::out_index(0, u) + tau;
        if (k >= w.klo && k < w.khi) st_stream(orow + k, v[u].re * scale);
    }
}

}  // namespace host
}  // namespace kofft
