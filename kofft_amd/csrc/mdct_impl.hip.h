// mdct_impl.hip.h -- the fast DCT-IV of rows of f32, the MDCT of rows of signals on it and the IMDCT's unfold-window-add (DESIGN.md
// 5.32).  The reference has no such entry point; every value is a composition of its operations, as include/kofft_hip.h states them.
//
// dct4_fast(u), N even, M = N / 2, c and d the two tables of kofft_hip_dct4_table_f32:
//   z[j] = (u[2j], u[N-1-2j]) * c[j]   Complex::mul un-fused (num.rs:162-165)
//   Z    = fft(z)                        (fft.rs:1054-1132; nothing for M == 1)
//   y[k] = Z[k] * d[k];  X[2k] = y[k].re, X[N-1-2k] = -y[k].im
// An IO policy names where u comes from -- rows of N reals (Dct4RowsIO), or the windowed and folded frames of rows of signals
// (MdctIO) -- and the dense rows of N reals that X goes to.  Two routes, the same operations per element:
//  * fused (M = 32 .. 4096, 4-byte aligned inputs, kofft_hip_set_mdct_fused on): dct4_fused_kernel<L, IO>, one pass over HBM on the
//    shared register transform (FusedGeom, fused_forward; fused_rows.hip.h), its stride-2 element pairs exchanged through LDS.  Items
//    of one workgroup may belong to different rows of signals, so the MDCT policy tests every sample against its own row's bounds
//    (plain loads, no shared descriptor);
//  * composed (every other N, unaligned inputs, the switch off): dct4_pre_kernel into the context's scratch, fft_dev in place,
//    dct4_post_kernel, in chunks of flat items.
// The IMDCT runs the DCT-IV of a chunk of frames into scratch by either route, then imdct_ola_kernel: one thread per output sample,
// reading its two values.
#pragma once

#include "frame_cut.h"
#include "fused_rows.hip.h"

namespace kofft {
namespace host {

// ---- IO policies: item(t) is computed once per thread (or element), pair(it, e) is (u[2e], u[N-1-2e]) of that item -------------
struct Dct4RowsIO {
    static constexpr bool kRowsLoad = true;
    const float *x;  // (x == out is allowed: every load of an item precedes its stores, and items do not share elements)
    float *out;
    size_t n;
    struct Item {
        const float *xr;
    };
    __device__ __forceinline__ Item item(size_t t) const { return Item{x + t * n}; }
    __device__ __forceinline__ cpx<float> pair(const Item &it, size_t e) const { return mk<float>(it.xr[2 * e], it.xr[n - 1 - 2 * e]); }
};

// Item t = row * frames + f: g[i] = x[f N + i - lead] * w[i] where that sample exists in its own row, +0 elsewhere (i < 2N); u is
// the fold of g.  No lane reads a sample of another row.
struct MdctIO {
    static constexpr bool kRowsLoad = false;
    const float *x, *w;
    float *out;
    size_t n, nx, row_stride, frames, lead;
    struct Item {
        const float *xr;
        long long first;  // the sample index of g[0]
    };
    __device__ __forceinline__ Item item(size_t t) const
    {
        const size_t row = t / frames, f = t - row * frames;
        return Item{x + row * row_stride, (long long)(f * n) - (long long)lead};
    }
    __device__ __forceinline__ float g(const Item &it, size_t i) const
    {
        const long long s = it.first + (long long)i;
        return (s >= 0 && s < (long long)nx) ? it.xr[s] * w[i] : 0.0f;
    }
    __device__ __forceinline__ float fold(const Item &it, size_t j) const
    {
        const size_t h = n / 2, q = n + h;  // N/2, 3N/2
        return j < h ? (-g(it, q - 1 - j)) - g(it, q + j) : g(it, j - h) - g(it, q - 1 - j);
    }
    __device__ __forceinline__ cpx<float> pair(const Item &it, size_t e) const { return mk<float>(fold(it, 2 * e), fold(it, n - 1 - 2 * e)); }
};

// y = Z[k] * d[k] goes to X[2k] and X[N-1-2k] of the item's output row
__device__ __forceinline__ void dct4_store(float *orow, const size_t n, const size_t k, const cpx<float> zk, const cpx<float> dk)
{
    const cpx<float> y = cmul(zk, dk);
    st_stream(orow + 2 * k, y.re);
    st_stream(orow + (n - 1 - 2 * k), -y.im);
}

// ---- composed route: flat grid-stride kernels, element e of a chunk is point e % M of item item0 + e / M ------------------------
template <class IO>
__global__ __launch_bounds__(256) void dct4_pre_kernel(const IO io, const cpx<float> *__restrict__ c, cpx<float> *__restrict__ z, const size_t m,
                                                       const size_t item0, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t q = e / m, j = e - q * m;
        const typename IO::Item it = io.item(item0 + q);
        st_stream(z + e, cmul(io.pair(it, j), c[j]));
    }
}

__global__ __launch_bounds__(256) void dct4_post_kernel(const cpx<float> *__restrict__ z, const cpx<float> *__restrict__ d, float *__restrict__ out,
                                                        const size_t m, const size_t item0, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t q = e / m, k = e - q * m;
        dct4_store(out + (item0 + q) * (2 * m), 2 * m, k, z[e], d[k]);
    }
}

// ---- fused route: M = 2^L, L = 5 .. 12 (N = 64 .. 8192) -----------------------------------------------------------------------------
// FusedGeom<L>::XPB items per 256-thread workgroup, TPT threads each.  Pass 0's register u of thread tau holds element e =
// in_index(0, u) + tau of z; after the transform register u holds bin k = out_index(0, u) | tau.  Element e needs u[2e] and u[N-1-2e]
// and bin k gives X[2k] and X[N-1-2k]: both pairs are stride 2 in memory, so rows of reals come in and every result goes out through
// one exchange in the item's LDS slot, TPT consecutive floats per instruction (kRowsLoad; the MDCT policy gathers its four products
// per pair straight from global memory).  A spare slot of the last workgroup transforms zeros and stores nothing.  (The last
// parameter is launch_fused_items' 1 / M, which this family does not use.)
template <int L, class IO>
__global__ __launch_bounds__(256) void dct4_fused_kernel(const IO io, const cpx<float> *__restrict__ c, const cpx<float> *__restrict__ d,
                                                         const cpx<float> *__restrict__ tw, const size_t items, const float)
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
    // The item's 2M reals pass through its LDS slot (2 lds_elems(M) >= 2M floats), so that the global loads of whole rows and every
    // global store are contiguous over tau instead of stride 2 (measured: DESIGN.md 5.32)
    float *fb = reinterpret_cast<float *>(smem_raw) + (size_t)slot * (2 * lds_elems(M));
    {
        const typename IO::Item it = io.item(live ? t : 0);
        cpx<float> raw[R], cv[R];
        if constexpr (IO::kRowsLoad) {
            float in[2 * R];
#pragma unroll
            for (int r = 0; r < 2 * R; ++r) in[r] = live ? it.xr[r * TPT + tau] : 0.0f;
#pragma unroll
            for (int r = 0; r < 2 * R; ++r) fb[r * TPT + tau] = in[r];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int e = G0::in_index(0, u) + tau;
                raw[u] = mk<float>(fb[2 * e], fb[2 * M - 1 - 2 * e]);
                cv[u] = c[e];
            }
            __syncthreads();  // (the transform's first exchange scatters into the same cells)
        } else {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int e = G0::in_index(0, u) + tau;
                raw[u] = live ? io.pair(it, (size_t)e) : mk<float>(0.0f, 0.0f);
                cv[u] = c[e];
            }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = cmul(raw[u], cv[u]);
    }
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    float *orow = io.out + t * (size_t)(2 * M);
    cpx<float> dv[R];
#pragma unroll
    for (int u = 0; u < R; ++u) dv[u] = d[GL::out_index(0, u) + tau];
    __syncthreads();  // every gather of the transform's last exchange is done
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int k = GL::out_index(0, u) + tau;
        const cpx<float> y = cmul(v[u], dv[u]);
        fb[2 * k] = y.re;
        fb[2 * M - 1 - 2 * k] = -y.im;
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 2 * R; ++r) st_stream(orow + r * TPT + tau, fb[r * TPT + tau]);
}

// ---- IMDCT: unfold, window, add ---------------------------------------------------------------------------------------------------------
// y_f[i] of a frame's v = dct4_fast(X_f): v[N/2 + i] for i < N/2, -v[3N/2 - 1 - i] for N/2 <= i < 3N/2, -v[i - 3N/2] beyond.
__device__ __forceinline__ float imdct_unfold(const float *v, const size_t n, const size_t i)
{
    const size_t h = n / 2, q = n + h;
    return i < h ? v[h + i] : (i < q ? -v[q - 1 - i] : -v[i - q]);
}

// One piece of a chunk (frame_cut.h): the frames [f0, ...) of rows [row, row + nr) lie dense at v, frame f0 of row `row` first, a
// row's frames `frames` apart when nr > 1 (then f0 == 0); where f0 > 0 the frame f0 - 1 lies right before v.  One thread per sample
// p in [lo, hi) of each row's `full`: block b = p / N, j = p % N,
//   full[p] = (w[N + j] * y_{b-1}[N + j] + w[j] * y_b[j]) * scale   where both frames exist, else the one product * scale,
// stored at out[(row + r) * out_len + p - out_first].
__global__ __launch_bounds__(256) void imdct_ola_kernel(const float *__restrict__ v, const float *__restrict__ w, float *__restrict__ out,
                                                        const size_t n, const size_t frames, const size_t row, const size_t f0, const size_t lo,
                                                        const size_t hi, const size_t out_first, const size_t out_len, const float scale,
                                                        const size_t total)
{
    const size_t span = hi - lo;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / span, p = lo + (e - r * span);
        const size_t b = p / n, j = p - b * n;
        const float *vb = v + (r * frames + (b - f0)) * n;  // frame b of row `row + r` (b == frames: one past the row's last)
        float acc;
        if (b == 0) acc = w[j] * imdct_unfold(vb, n, j);
        else if (b == frames) acc = w[n + j] * imdct_unfold(vb - n, n, n + j);
        else acc = w[n + j] * imdct_unfold(vb - n, n, n + j) + w[j] * imdct_unfold(vb, n, j);
        st_stream(out + (row + r) * out_len + (p - out_first), acc * scale);
    }
}

}  // namespace host
}  // namespace kofft
