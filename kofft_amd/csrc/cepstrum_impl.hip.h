// cepstrum_impl.hip.h -- cepstrum::real_cepstrum (cepstrum.rs:12-33) on device pointers, f32 only like the reference.
//
// For a row of n reals (n a power of two; anything else is the reference's NonPowerOfTwoNoStd) the reference computes
//   freq = fft((x, +0));  every bin: mag = sqrtf(re * re + im * im), re = logf(mag + 1e-12f), im = +0;  out = ifft(freq).re
// with ifft = conj (im = -im), fft, conj, * (1 / n) and an early return at n == 1 (fft.rs:1134-1174).  The magnitude is the sum of
// squares as written (two multiplies and an add, unfused, then a correctly rounded root: not hypotf), and logf is the libm crate's
// (libm_logf.hip.h).  The pointwise step is the same for every bin, so no bin position enters it.  Two routes, the same operations
// per element:
//  * fused (powers of two n = 32 .. 4096): cepstrum_fused_kernel<L>, one pass over HBM.  hilbert_fused_kernel's body
//    (fused_two_transforms, fused_rows.hip.h) with the policy CepstrumFused: rows load as (x, +0) through one buffer
//    descriptor per workgroup, the forward transform runs, the last pass's registers take log-magnitude + conj, one LDS exchange
//    puts them back into pass-0 input order, the same forward transform runs again and the store writes re * scale only, 4 bytes
//    per point;
//  * composed (n <= 16, 8192 .. 2^26, inputs that are not 4-byte aligned, and every n after kofft_hip_set_cepstrum_fused(ctx, 0)):
//    the output holds only n floats per row, so the context's real scratch is the workspace, in row chunks of 512 MiB at most --
//    expand_real_kernel writes (x, +0), fft_dev transforms in place, cepstrum_logmag_kernel, fft_dev(inverse) runs the
//    reference's ifft in place, cepstrum_real_kernel takes the real parts into the output.
// Both routes read all of a row before they write any of it: in == out is allowed; a partial overlap is undefined.
#pragma once

#include "fused_rows.hip.h"
#include "libm_logf.hip.h"

namespace kofft {
namespace host {

// cepstrum.rs:27-29 on one bin: the log-magnitude, as (re, im = +0)
__device__ __forceinline__ float cepstrum_log_mag(const cpx<float> c)
{
    const float mag = sqrtf(c.re * c.re + c.im * c.im);
    return libm_logf(mag + 1e-12f);  // 1e-12f: 0x2b8cbccc
}

// ---- composed route ---------------------------------------------------------------------------------------------------------
// Flat grid-stride grids over the whole chunk, as hilbert_mask_kernel: every bin takes the same operations.
__global__ __launch_bounds__(256) void cepstrum_logmag_kernel(cpx<float> *__restrict__ z, const size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) z[i] = mk<float>(cepstrum_log_mag(z[i]), 0.0f);
}

// cepstrum.rs:32: the real parts
__global__ __launch_bounds__(256) void cepstrum_real_kernel(const cpx<float> *__restrict__ z, float *__restrict__ out, const size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) st_stream(out + i, z[i].re);
}

inline int cepstrum_composed_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    // rows per chunk as dct2_composed_dev: scratch_chunk_bytes of scratch at most
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, n * sizeof(cpx<float>), batch);
    const int rc = ensure(ctx, ctx->real_tmp, chunk * n * sizeof(cpx<float>));
    if (rc) return rc;
    float *zf = static_cast<float *>(ctx->real_tmp.p);
    cpx<float> *z = static_cast<cpx<float> *>(ctx->real_tmp.p);
    return for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
        const size_t total = n * nb;
        const dim3 grid(flat_blocks(ctx, total, 64));
        hipLaunchKernelGGL(expand_real_kernel, grid, dim3(256), 0, ctx->stream, d_in + b0 * n, z, total);  // cepstrum.rs:20-23
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (n > 1) {  // (n == 1: the transform is nothing, fft.rs:1059)
            const int frc = fft_dev<float>(ctx, zf, zf, n, nb, 0);  // cepstrum.rs:25
            if (frc) return frc;
        }
        hipLaunchKernelGGL(cepstrum_logmag_kernel, grid, dim3(256), 0, ctx->stream, z, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (n > 1) {  // (n == 1: ifft returns early, fft.rs:1139)
            const int irc = fft_dev<float>(ctx, zf, zf, n, nb, 1);  // cepstrum.rs:31: conj, fft, conj * (1 / n)
            if (irc) return irc;
        }
        hipLaunchKernelGGL(cepstrum_real_kernel, grid, dim3(256), 0, ctx->stream, z, d_out + b0 * n, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return KOFFT_OK;
    });
}

// ---- fused route: powers of two n = 2^L, L = 5 .. 12 ------------------------------------------------------------------------
// every bin: (log-magnitude, +0), then ifft's conj (fft.rs:1163-1165): (l, -0); the store: ifft's conj leaves the real part
// alone, * scale (fft.rs:1168-1172), real part only
struct CepstrumFused {
    using Out = float;
    template <int N>
    static __device__ __forceinline__ void point(cpx<float> &v, int, int) { v = mk<float>(cepstrum_log_mag(v), -0.0f); }
    static __device__ __forceinline__ void store(const cpx<float> v, const float scale, const rsrc_t d, const int lane_bytes, const int off)
    {
        buf_store_f32(v.re * scale, d, lane_bytes, off);
    }
};

template <int L>
__global__ __launch_bounds__(256) void cepstrum_fused_kernel(const float *__restrict__ x, float *__restrict__ out, const cpx<float> *__restrict__ tw,
                                                             const size_t batch, const float scale)
{
    fused_two_transforms<L, CepstrumFused>(x, out, tw, batch, scale);
}

}  // namespace host
}  // namespace kofft
