// planar_impl.hip.h -- FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on device pointers: the transform of rows whose real and
// imaginary parts lie in two separate planes ("planar", the reference's SoA / SplitComplex / ComplexVec layout), f32 and f64.
//
// fft_split(re, im) packs lengths that are not a power of two, and n <= 16, into Complex values and calls fft (fft.rs:797-808); every
// other length runs the radix-2 Stockham stages of fft.rs:834-898 / 959-1037 on the two arrays -- the butterflies, the get_twiddles(n)
// table and the operation order of fft on interleaved data.  ifft_split negates im, runs the same, then im = -im, re *= scale,
// im *= scale (fft.rs:1393-1428): ifft's conj, fft, conj, scale.  So re_out + i im_out is fft / ifft of re + i im bit for bit, and the
// layout is one more IO policy of the kernels of fft_wg.hip.h.  (n == 1: ifft returns early, ifft_split negates twice and multiplies
// by 1.0 -- the value itself unless it is a NaN; the planes are copied.)  Two routes, the same operations per element:
//  * fused (powers of two n = 2 .. 2^14 in f32, 2 .. 2^13 in f64): PlanarIO in fft_small_kernel (n <= 16, f32 n = 32) or fft_wg_kernel,
//    the geometry of the complex transform of that n -- one launch, every value crosses HBM once each way;
//  * composed (every other length fft_dev takes, and every n after kofft_hip_set_split_fused(ctx, 0)): planar_pack_kernel writes
//    interleaved rows into the context's scratch, fft_dev transforms them in place, planar_unpack_kernel stores the two planes.
// Nothing here is called "split" in kernel code: fft_split.hip.h is the wave-split kernels.
#pragma once

#include "host_common.hip.h"
#include "host_stage.hip.h"

namespace kofft {

template <typename T>
__device__ __forceinline__ T ld_plane(const T *p)
{
    return __builtin_nontemporal_load(p);
}
template <typename T>
__device__ __forceinline__ void st_plane(T *p, T v)
{
    __builtin_nontemporal_store(v, p);
}

// Element i of transform xf is re_in[xf * n + i], im_in[xf * n + i]; plain per-element 4- / 8-byte accesses, coalesced over the lanes
// of a transform (kStreams = false: no descriptor forms; kPersist = false: the one-tile-per-workgroup kernels only).  No __restrict__:
// re_in == re_out and im_in == im_out is the reference's own in-place form, and the kernels read a whole transform (fft_small_kernel: a
// whole workgroup's rows) before a barrier and write it after.  No store here is wider than 8 bytes, so the f64 16-byte store hazard
//  has nothing to act on.
template <typename T, bool INVERSE>
struct PlanarIO : PlainTw {
    static constexpr int kSmallBlock16 = ComplexIO<T, INVERSE>::kSmallBlock16;  // the complex transform's geometry at every n
    static constexpr bool kStreams = false;
    static constexpr bool kPersist = false;
    static constexpr bool kInvInLds = false;
    static constexpr bool kLeanRegisters = true;
    static constexpr bool kLen1 = false;  // planar_dev copies a one-point transform
    using Raw = cpx<T>;
    using Inv = NoInv;
    const T *re_in, *im_in;
    T *re_out, *im_out;
    int n;
    T scale;  // 1 / (n as f32 as T), fft.rs:1167
    __device__ __forceinline__ Raw fetch(size_t xf, int i) const
    {
        const size_t e = xf * (size_t)n + i;
        return mk<T>(ld_plane(re_in + e), ld_plane(im_in + e));
    }
    __device__ __forceinline__ cpx<T> finish(size_t, int, Raw v, Inv) const
    {
        if (INVERSE) v.im = -v.im;  // fft.rs:1400-1402
        return v;
    }
    __device__ __forceinline__ cpx<T> load(size_t xf, int i) const { return finish(xf, i, fetch(xf, i), {}); }
    __device__ __forceinline__ void store(size_t xf, int o, cpx<T> v) const
    {
        if (INVERSE) {  // fft.rs:1405-1409
            const T im = -v.im;
            v.re = v.re * scale;
            v.im = im * scale;
        }
        const size_t e = xf * (size_t)n + o;
        st_plane(re_out + e, v.re);
        st_plane(im_out + e, v.im);
    }
};

namespace host {

// ---- composed route ---------------------------------------------------------------------------------------------------------
// Flat grids over a chunk of rows (rows back to back in both layouts, so element e of the chunk is element e of each plane); the grid
// strides over chunks larger than it.
template <typename T>
__global__ __launch_bounds__(256) void planar_pack_kernel(const T *re, const T *im, cpx<T> *z, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) st_stream(z + e, mk<T>(ld_plane(re + e), ld_plane(im + e)));
}

template <typename T>
__global__ __launch_bounds__(256) void planar_unpack_kernel(const cpx<T> *z, T *re, T *im, const size_t total)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const cpx<T> v = ld_stream(z + e);
        st_plane(re + e, v.re);
        st_plane(im + e, v.im);
    }
}

template <typename T>
int planar_composed_dev(kofft_hip_ctx *ctx, const T *re_in, const T *im_in, T *re_out, T *im_out, size_t n, size_t batch, int inverse)
{
    // rows per chunk as dct2_composed_dev: scratch_chunk_bytes of interleaved scratch at most (one row where a row is longer)
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, n * sizeof(cpx<T>), batch);
    int rc = ensure(ctx, ctx->real_tmp, chunk * n * sizeof(cpx<T>));
    if (rc) return rc;
    cpx<T> *z = static_cast<cpx<T> *>(ctx->real_tmp.p);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t nb = (batch - b0 < chunk) ? batch - b0 : chunk, total = nb * n, off = b0 * n;
        const dim3 grid(flat_blocks(ctx, total, 64));
        hipLaunchKernelGGL(planar_pack_kernel<T>, grid, dim3(256), 0, ctx->stream, re_in + off, im_in + off, z, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        rc = fft_dev<T>(ctx, reinterpret_cast<T *>(z), reinterpret_cast<T *>(z), n, nb, inverse);
        if (rc) return rc;
        hipLaunchKernelGGL(planar_unpack_kernel<T>, grid, dim3(256), 0, ctx->stream, z, re_out + off, im_out + off, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------------
// Lengths the fused route takes in a context that has it on: the powers of two of the one-workgroup kernels.  (the
// measured table decides which of them stay here.)
template <typename T>
inline bool planar_fused_ok(const kofft_hip_ctx *ctx, size_t n)
{
    return ctx->planar_fused && is_pow2(n) && n >= 2 && n <= (size_t(1) << max_log2<T>());
}

// the argument checks alone, in the order of fft_dev and before the context or a device is touched
inline int planar_check(size_t n, size_t batch, const void *p0, const void *p1, const void *p2, const void *p3, const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;  // fft.rs:794
    if (!complex_len_ok(n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !p0 || !p1 || !p2 || !p3) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

template <typename T>
int planar_dev(kofft_hip_ctx *ctx, const T *re_in, const T *im_in, T *re_out, T *im_out, size_t n, size_t batch, int inverse)
{
    const int crc = planar_check(n, batch, re_in, im_in, re_out, im_out, ctx);
    if (crc || batch == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 1) {  // fft.rs:1059: nothing; ifft_split: -(-im), * 1.0 -- the planes themselves
        if (re_in != re_out) KOFFT_HIP_TRY(ctx, hipMemcpyAsync(re_out, re_in, batch * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        if (im_in != im_out) KOFFT_HIP_TRY(ctx, hipMemcpyAsync(im_out, im_in, batch * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        return KOFFT_OK;
    }
    if (!planar_fused_ok<T>(ctx, n)) return planar_composed_dev<T>(ctx, re_in, im_in, re_out, im_out, n, batch, inverse);
    const T scale = (T)1 / (T)(float)n;  // fft.rs:1167
    if (inverse) {
        PlanarIO<T, true> io{{}, re_in, im_in, re_out, im_out, (int)n, scale};
        return dispatch<T, EPI_STORE>(ctx, io, n, batch);
    }
    PlanarIO<T, false> io{{}, re_in, im_in, re_out, im_out, (int)n, scale};
    return dispatch<T, EPI_STORE>(ctx, io, n, batch);
}

// the same on host planes of batch * n reals each, in place
template <typename T>
int planar_host(kofft_hip_ctx *ctx, T *re, T *im, size_t n, size_t batch, int inverse)
{
    const int crc = planar_check(n, batch, re, im, re, im, ctx);
    if (crc || batch == 0) return crc;
    if (n == 1) return KOFFT_OK;  // the planes themselves
    const HostArray<T> a[2] = {{re, re, n}, {im, im, n}};
    return rows_host_n<T>(ctx, batch, 2, a, nullptr, 0, is_pow2(n), true,
                          [&](T *const *d, const T *, size_t nb) { return planar_dev<T>(ctx, d[0], d[1], d[0], d[1], n, nb, inverse); });
}

}  // namespace host
}  // namespace kofft
