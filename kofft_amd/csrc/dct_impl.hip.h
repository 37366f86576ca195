// dct_impl.hip.h -- DctPlanner::plan_dct2 (dct.rs:61-105) on device pointers, f32 only like the reference.
//
// dct2_with_table mirrors each row of n reals into 2n (buf[i] = buf[2n-1-i] = x[i], dct.rs:77-80), takes rfft_direct of
// the 2n reals (dct.rs:86; rfft.rs:425-465 with m = n) and twists bins 0 .. n-1 (dct.rs:87-92):
//   out[k] = 0.5 * (spec[k].re * cos[k] + spec[k].im * sin[k]),  (cos, sin)[k] of a_k = PI * k / (2n)  (tables.cpp)
// Two routes, the same operations per element:
//  * fused (powers of two n = 32 .. 4096): dct2_fused_kernel<L>, one pass over HBM -- the mirror on the load, the reference's
//    radix-2 Stockham stages (fft.rs:790-911: the arm ScalarFftImpl::fft takes for powers of two from 32) in LDS, the post-pass
//    and the twist on the way out;
//  * composed (everything else: n <= 16, whose transforms are the reference's straight-line kernels, powers of two above 4096,
//    other lengths, unaligned inputs; and every n after kofft_hip_set_dct_fused(ctx, 0)): dct2_mirror_kernel writes the mirrored rows (read as n complex
//    values: rfft.rs:444-446's packing) into scratch, fft_dev runs the n-point complex transform in place (every route of the
//    library: Bluestein for odd n, the factor path for large powers of two), dct2_post_kernel does the post-pass of
//    rfft.rs:450-463 with rfft_post_one's expressions and the twist.
// Bin n of the rfft is never formed (the reference computes it and does not read it).
#pragma once

#include "real_impl.hip.h"

namespace kofft {
namespace host {

// z[b] = mirrored row b as n complex values: z[p] = (x[2p], x[2p+1]) and z[n-1-p] = (x[2p+1], x[2p]), p < n/2 (n even);
// odd n: the middle value (x[n-1], x[n-1]).  grid.x covers p, grid.y walks the rows: no division per element.  vec: 8-byte
// loads (n even and x 8-byte aligned), else two 4-byte loads.
// Short rows (n < 512: a 256-thread block per row would idle) run flat: one thread per (row, p) over the chunk, 32-bit index
// math (a chunk holds at most 2^27 floats).
__device__ __forceinline__ bool dct2_flat_item(const size_t n, const size_t rows, size_t &b, size_t &p)
{
    const unsigned per = (unsigned)(n / 2 + 1), i = blockIdx.x * 256u + threadIdx.x;
    if ((size_t)i >= rows * per) return false;
    b = i / per;
    p = i % per;
    return true;
}
__global__ __launch_bounds__(256) void dct2_mirror_kernel(const float *__restrict__ x, cpx<float> *__restrict__ z, const size_t n, const size_t rows,
                                                          const bool vec, const bool flat)
{
    size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y, bstep = gridDim.y;
    if (flat) {
        if (!dct2_flat_item(n, rows, b0, p)) return;
        bstep = rows;
    }
    const size_t half = n / 2;
    if (p > half || (p == half && !(n & 1))) return;
    for (size_t b = b0; b < rows; b += bstep) {
        const float *xr = x + b * n;
        cpx<float> *zr = z + b * n;
        if (p == half) {  // odd n: buf[n-1] = buf[n] = x[n-1]
            const float v = xr[n - 1];
            zr[half] = mk<float>(v, v);
        } else if (vec) {
            const float2 v = *reinterpret_cast<const float2 *>(xr + 2 * p);
            zr[p] = mk<float>(v.x, v.y);
            zr[n - 1 - p] = mk<float>(v.y, v.x);
        } else {
            const float a = xr[2 * p], c = xr[2 * p + 1];
            zr[p] = mk<float>(a, c);
            zr[n - 1 - p] = mk<float>(c, a);
        }
    }
}

// dct.rs:91: 0.5 * (re * cos + im * sin), un-fused (-ffp-contract=off)
__device__ __forceinline__ float dct2_twist(const cpx<float> s, const cpx<float> cs)
{
    return 0.5f * (s.re * cs.re + s.im * cs.im);
}

// out[0] from Y[0] (rfft.rs:450: output[0] = (y0.re + y0.im, 0)); out[j], out[n-j] from Y[j], Y[n-j] (rfft.rs:454-463)
__device__ __forceinline__ void dct2_post_pair(const cpx<float> *__restrict__ rtab, const cpx<float> *__restrict__ cs, float *orow,
                                               const size_t n, const size_t j, const cpx<float> a, const cpx<float> c)
{
    if (j == 0) {
        orow[0] = dct2_twist(mk<float>(a.re + a.im, 0.0f), cs[0]);
    } else {  // (n even: j = n/2 pairs with itself)
        orow[j] = dct2_twist(rfft_post_one<float>(a, c, rtab[j]), cs[j]);
        if (n - j != j) orow[n - j] = dct2_twist(rfft_post_one<float>(c, a, rtab[n - j]), cs[n - j]);
    }
}

// One thread per bin pair (j, n - j), j = 0 .. n/2; grid.x covers j, grid.y walks the rows: Y[j] and Y[n-j] are read once.
__global__ __launch_bounds__(256) void dct2_post_kernel(const cpx<float> *__restrict__ y, const cpx<float> *__restrict__ rtab,
                                                        const cpx<float> *__restrict__ cs, float *__restrict__ out, const size_t n,
                                                        const size_t rows, const bool flat)
{
    size_t j = (size_t)blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y, bstep = gridDim.y;
    if (flat) {
        if (!dct2_flat_item(n, rows, b0, j)) return;
        bstep = rows;
    }
    if (j > n / 2) return;
    for (size_t b = b0; b < rows; b += bstep) {
        const cpx<float> *yr = y + b * n;
        dct2_post_pair(rtab, cs, out + b * n, n, j, yr[j], yr[j == 0 ? 0 : n - j]);
    }
}

// ---- fused route: powers of two n = 2^L, L = 5 .. 12 ------------------------------------------------------------------------
// One 256-thread workgroup per R = max(1, 512 / n) rows.  The rows' mirrored packed values go into LDS straight from the input
// (each input pair read once, 8-byte loads), the twiddles get_twiddles(n) (n/2 entries) beside them.  Stage s of the reference's
// Stockham loop (fft.rs:836-898; n1 = 2^s, n2 = n / 2^(s+1)): butterfly q = k * n2 + j reads e = src[2k n2 + j], o = src[2k n2 +
// n2 + j], forms t = o * T[k n2] as 4 mul + 1 sub + 1 add and writes dst[q] = e + t, dst[q + n/2] = e - t -- every thread first
// reads its butterflies' inputs, then (after a barrier) writes, so one buffer serves as source and destination.  Which thread runs
// which butterfly does not change any value.  The post-pass and the twist read Y from LDS and store n reals per row.
template <int L>
constexpr int dct2_fused_rows() { return (1 << L) >= 512 ? 1 : 512 >> L; }
template <int L>
constexpr size_t dct2_fused_lds_bytes() { return ((size_t)dct2_fused_rows<L>() * (1 << L) + (1 << (L - 1))) * sizeof(cpx<float>); }

template <int L>
__global__ __launch_bounds__(256) void dct2_fused_kernel(const float *__restrict__ x, const cpx<float> *__restrict__ tw,
                                                         const cpx<float> *__restrict__ rtab, const cpx<float> *__restrict__ cs,
                                                         float *__restrict__ out, const size_t batch)
{
    constexpr int N = 1 << L, H = N / 2, R = dct2_fused_rows<L>(), P = R * N;
    constexpr int BPT = (R * H) / 256;  // butterflies per thread and stage (>= 1: R * H >= 256)
    static_assert(BPT >= 1 && (R * H) % 256 == 0, "whole butterflies per thread");
    extern __shared__ cpx<float> dct2_lds[];
    cpx<float> *buf = dct2_lds, *tws = dct2_lds + P;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * R;
    for (int i = tid; i < H; i += 256) tws[i] = tw[i];
    // the mirror (dct.rs:77-80) as rfft.rs:444-446 packs it: xc[p] = (x[2p], x[2p+1]) at p and, swapped, at N-1-p
    for (int g = tid; g < R * H; g += 256) {
        const int r = g / H, p = g % H;  // (compile-time powers of two: shifts)
        cpx<float> v = mk<float>(0.0f, 0.0f);
        if (row0 + r < batch) {
            const float2 f = *reinterpret_cast<const float2 *>(x + (row0 + r) * N + 2 * p);
            v = mk<float>(f.x, f.y);
        }
        buf[r * N + p] = v;
        buf[r * N + N - 1 - p] = mk<float>(v.im, v.re);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < L; ++s) {
        const int n2 = N >> (s + 1);
        cpx<float> e[BPT], o[BPT], w[BPT];
#pragma unroll
        for (int u = 0; u < BPT; ++u) {
            const int g = tid + 256 * u, r = g / H, q = g % H, k = q / n2, j = q % n2;
            const int base = r * N + 2 * k * n2 + j;
            e[u] = buf[base];
            o[u] = buf[base + n2];
            w[u] = tws[k * n2];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < BPT; ++u) {
            const int g = tid + 256 * u, r = g / H, q = g % H;
            const float t_re = o[u].re * w[u].re - o[u].im * w[u].im;
            const float t_im = o[u].re * w[u].im + o[u].im * w[u].re;
            buf[r * N + q] = mk<float>(e[u].re + t_re, e[u].im + t_im);
            buf[r * N + q + H] = mk<float>(e[u].re - t_re, e[u].im - t_im);
        }
        __syncthreads();
    }
    for (int g = tid; g < R * (H + 1); g += 256) {
        const int r = g / (H + 1), j = g % (H + 1);
        if (row0 + r >= batch) continue;
        const cpx<float> *yr = buf + r * N;
        dct2_post_pair(rtab, cs, out + (row0 + r) * N, N, j, yr[j], yr[j == 0 ? 0 : N - j]);
    }
}

template <int L>
int launch_dct2_fused(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const cpx<float> *tw, const cpx<float> *rtab,
                      const cpx<float> *cs, size_t batch)
{
    constexpr int R = dct2_fused_rows<L>();
    constexpr size_t lds = dct2_fused_lds_bytes<L>();
    static_assert(lds <= 64 * 1024, "LDS budget");
    const size_t blocks = (batch + R - 1) / R;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dct2_fused_kernel<L>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, d_in, tw, rtab, cs, d_out, batch);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// (the kernel's 8-byte loads need an 8-byte aligned input; a caller's pointer that is not takes the composed route)
inline bool dct2_fused_ok(const kofft_hip_ctx *ctx, const float *d_in, size_t n)
{
    return ctx->dct_fused && is_pow2(n) && n >= 32 && n <= 4096 && (reinterpret_cast<size_t>(d_in) & 7) == 0;
}

inline int dct2_fused_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const cpx<float> *tw = nullptr, *rtab = nullptr, *cs = nullptr;
    int rc = twiddle_table<float>(ctx, n, &tw);  // get_twiddles(n), the table of the n-point transform
    if (rc) return rc;
    rc = rfft_table<float>(ctx, n, &rtab);
    if (rc) return rc;
    rc = dct2_table(ctx, n, &cs);
    if (rc) return rc;
    // (never outside 5 .. 12: dct2_fused_ok)
    return dispatch_log2<5, 12>(ilog2(n), [&](auto l) { return launch_dct2_fused<decltype(l)::value>(ctx, d_in, d_out, tw, rtab, cs, batch); });
}

inline int dct2_composed_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const cpx<float> *rtab = nullptr, *cs = nullptr;
    int rc = rfft_table<float>(ctx, n, &rtab);  // build_twiddle_table(m = n) of the 2n-real rfft
    if (rc) return rc;
    rc = dct2_table(ctx, n, &cs);
    if (rc) return rc;
    // rows per chunk as rfft_composed_dev, counted on the mirrored 2n-real rows: scratch_chunk_bytes of scratch at most
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, 2 * n * sizeof(float), batch);
    rc = ensure(ctx, ctx->real_tmp, chunk * n * sizeof(cpx<float>));
    if (rc) return rc;
    float *z = static_cast<float *>(ctx->real_tmp.p);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t nb = (batch - b0 < chunk) ? batch - b0 : chunk;
        const bool flat = n < 512;
        const dim3 grid = flat ? dim3(blocks_for(nb * (n / 2 + 1))) : dim3(blocks_for(n / 2 + 1), (unsigned)(nb < 65535 ? nb : 65535));
        hipLaunchKernelGGL(dct2_mirror_kernel, grid, dim3(256), 0, ctx->stream, d_in + b0 * n, reinterpret_cast<cpx<float> *>(z), n, nb,
                           !(n & 1) && (reinterpret_cast<size_t>(d_in) & 7) == 0, flat);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        rc = fft_dev<float>(ctx, z, z, n, nb, 0);  // dct.rs:86 -> rfft.rs:447: fft.fft(&mut output[..m]), m = n
        if (rc) return rc;
        hipLaunchKernelGGL(dct2_post_kernel, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const cpx<float> *>(z), rtab, cs,
                           d_out + b0 * n, n, nb, flat);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft
