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
//    HBM, on the register-pass machinery of the Hilbert / cepstrum kernels (HilbertGeom, hilbert_forward; hilbert_impl.hip.h).  It
//    keeps its own body: items of one workgroup may belong to different rows, so every lane tests its own sample against its own
//    row's bounds (plain loads, no shared descriptor), and the store keeps a part of each frame only;
//  * composed (every other block up to 65536, unaligned inputs, the switch off): convolve_expand_kernel into the context's scratch,
//    fft_dev, convolve_mul_kernel, fft_dev(inverse), convolve_gather_kernel, in chunks of flat items (a seam may fall inside a row).
// The filter spectra are computed first on every call: convolve_filter_kernel, then fft_dev in place, at the head of the scratch.
// x / h and out must not overlap.
#pragma once

#include "hilbert_impl.hip.h"

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

// ---- filter spectra, composed route -------------------------------------------------------------------------------------------
// Flat grid-stride kernels as the Hilbert composed route's: element e of a chunk is point e & (block - 1) of item e >> lb.
__global__ __launch_bounds__(256) void convolve_filter_kernel(const float *__restrict__ h, cpx<float> *__restrict__ H, const size_t nh,
                                                              const int lb, const int reverse, const size_t total)
{
    const size_t mask = (size_t(1) << lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t f = e >> lb, i = e & mask;
        float v = 0.0f;
        if (i < nh) v = h[f * nh + (reverse ? nh - 1 - i : i)];
        H[e] = mk<float>(v, 0.0f);
    }
}

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

__global__ __launch_bounds__(256) void convolve_gather_kernel(const cpx<float> *__restrict__ z, float *__restrict__ out, const ConvShape s,
                                                              const size_t item0, const size_t total)
{
    const size_t mask = (size_t(1) << s.lb) - 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t it = item0 + (e >> s.lb), i = e & mask;
        if (i < s.nh - 1) continue;
        const size_t row = s.row_of(it), b = s.b0 + (it - row * s.nbw);
        const size_t pos = b * s.hop + (i - (s.nh - 1));
        if (pos >= s.out_first && pos - s.out_first < s.out_len) st_stream(out + row * s.out_len + (pos - s.out_first), z[e].re);
    }
}

// ---- fused route: block = 2^L, L = 5 .. 12 --------------------------------------------------------------------------------------
// HilbertGeom<L>::XPB items per 256-thread workgroup, TPT threads each.  Pass 0's register u of thread tau holds element
// in_index(0, u) + tau of its item's frame; after each transform register u holds bin out_index(0, u) | tau.
template <int L>
__global__ __launch_bounds__(256) void convolve_fused_kernel(const float *__restrict__ x, const cpx<float> *__restrict__ H, float *__restrict__ out,
                                                             const cpx<float> *__restrict__ tw, const ConvShape s, const float scale)
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
    cpx<float> v[R];
    {
        // elements [lo, hi) of the frame are samples of this row: block 0's leading zeros and the zeros past nx come from the test,
        // no lane reads outside its row
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
        for (int u = 0; u < R; ++u) v[u] = mk<float>(raw[u], 0.0f);
    }
    hilbert_forward<L>(v, smem_raw, tw, tau, slot);
    {   // Y = X * H (num.rs:162-165), then ifft's conj (fft.rs:1163-1165)
        const cpx<float> *Hr = H + (s.per_row ? row : 0) * (size_t)N + tau;
        cpx<float> hv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) hv[u] = Hr[GL::out_index(0, u)];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const cpx<float> y = cmul(v[u], hv[u]);
            v[u] = mk<float>(y.re, -y.im);
        }
    }
    {   // last pass's output order -> pass 0's input order, through the item's exchange slot
        cpx<float> *buf = reinterpret_cast<cpx<float> *>(smem_raw) + (size_t)slot * lds_elems(N);
        __syncthreads();  // every gather of the transform's last exchange is done
#pragma unroll
        for (int u = 0; u < R; ++u) buf[lds_pad(GL::out_index(tau, u))] = v[u];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = buf[lds_pad(G0::in_index(tau, u))];
        __syncthreads();  // (the second transform's first exchange scatters into the same cells)
    }
    hilbert_forward<L>(v, smem_raw, tw, tau, slot);
    // Element k of y goes to full_out[b * hop + k - (nh - 1)] for k >= nh - 1; kept where that lies inside the row's window:
    // k in [klo, khi).  ifft's last conj leaves the real part alone; * scale (fft.rs:1168-1172).
    const long long shift = (long long)(b * s.hop) - (long long)(s.nh - 1) - (long long)s.out_first;  // window index = k + shift
    const long long lo64 = -shift > (long long)(s.nh - 1) ? -shift : (long long)(s.nh - 1);
    const long long hi64 = (long long)s.out_len - shift;
    const int klo = lo64 < (long long)N ? (int)lo64 : N;
    const int khi = !live || hi64 <= 0 ? 0 : (hi64 < (long long)N ? (int)hi64 : N);
    float *orow = out + row * s.out_len + shift;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int k = GL::out_index(0, u) + tau;
        if (k >= klo && k < khi) st_stream(orow + k, v[u].re * scale);
    }
}

template <int L>
int launch_convolve_fused(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, float *d_out, const cpx<float> *tw, const ConvShape &s)
{
    using Geo = HilbertGeom<L>;
    constexpr size_t lds = Geo::lds_bytes();
    static_assert(lds <= 64 * 1024, "LDS budget");
    const size_t blocks = (s.items + Geo::XPB - 1) / Geo::XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    const float scale = 1.0f / (float)Geo::N;  // fft.rs:1167
    hipLaunchKernelGGL(convolve_fused_kernel<L>, dim3((unsigned)blocks), dim3(Geo::BLOCK), lds, ctx->stream, d_x, H, d_out, tw, s, scale);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft
