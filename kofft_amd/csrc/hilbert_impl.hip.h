// hilbert_impl.hip.h -- hilbert::hilbert_analytic (hilbert.rs:13-47) on device pointers, f32 only like the reference.
//
// For a row of n reals (n a power of two; anything else is the reference's NonPowerOfTwoNoStd) the reference computes
//   freq = fft((x, +0));  bins 1 .. n/2-1: re *= 2, im *= 2;  bins n/2+1 .. n-1 = (+0, +0);  out = ifft(freq)
// with ifft = conj (im = -im), fft, conj, * (1 / n) and an early return at n == 1 (fft.rs:1134-1174).  The mask is two real
// multiplies (an Inf stays an Inf; a complex multiply by (2, 0) would make NaNs), and the conj is a negation, so a zeroed bin
// enters the second transform as (+0, -0).  Two routes, the same operations per element:
//  * fused (powers of two n = 32 .. 4096): hilbert_fused_kernel<L>, one pass over HBM.  Its body is fused_two_transforms
//    (fused_rows.hip.h), which the cepstrum's fused kernel shares, with the policy HilbertFused: rows load as (x, +0) through one
//    buffer descriptor per workgroup, the forward transform runs, the last pass's registers -- whose bins the geometry names at
//    compile time up to the thread's low bits -- take mask + conj, one LDS exchange puts them back into pass-0 input order, the
//    same forward transform runs again and the store applies conj * scale;
//  * composed (n <= 16, whose transforms are the reference's straight-line kernels, powers of two above 4096, inputs that are not
//    4-byte aligned, and every n after kofft_hip_set_hilbert_fused(ctx, 0)): the caller's output is the workspace --
//    expand_real_kernel writes (x, +0), fft_dev transforms in place, hilbert_mask_kernel masks, fft_dev(inverse) runs the
//    reference's ifft in place.
#pragma once

#include "fused_rows.hip.h"

namespace kofft {
namespace host {

// ---- composed route ---------------------------------------------------------------------------------------------------------
// Flat grids over the whole batch as expand_real_kernel's (rows back to back; n is a power of two, so a sample's bin is its index's
// low bits).
// hilbert.rs:28-34 (n even, n >= 4): bins 0 and n/2 untouched, 1 .. n/2-1 doubled part by part, n/2+1 .. n-1 = Complex32::zero()
__global__ __launch_bounds__(256) void hilbert_mask_kernel(cpx<float> *__restrict__ z, const size_t n, const size_t total)
{
    const size_t h = n / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t j = i & (n - 1);
        if (j == 0 || j == h) continue;
        if (j < h) {
            const cpx<float> v = z[i];
            z[i] = mk<float>(v.re * 2.0f, v.im * 2.0f);
        } else {
            z[i] = mk<float>(0.0f, 0.0f);
        }
    }
}

inline int hilbert_composed_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    cpx<float> *z = reinterpret_cast<cpx<float> *>(d_out);
    const size_t total = n * batch;
    hipLaunchKernelGGL(expand_real_kernel, dim3(flat_blocks(ctx, total, 64)), dim3(256), 0, ctx->stream, d_in, z, total);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    if (n == 1) return KOFFT_OK;  // fft: nothing (fft.rs:1059); n odd: no mask; ifft returns early (fft.rs:1139)
    int rc = fft_dev<float>(ctx, d_out, d_out, n, batch, 0);  // hilbert.rs:25
    if (rc) return rc;
    if (n > 2) {  // (n = 2: bins 1 .. 0 and 2 .. 1 -- nothing to mask)
        hipLaunchKernelGGL(hilbert_mask_kernel, dim3(flat_blocks(ctx, total, 64)), dim3(256), 0, ctx->stream, z, n, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return fft_dev<float>(ctx, d_out, d_out, n, batch, 1);  // hilbert.rs:45: conj, fft, conj * (1 / n)
}

// ---- fused route: powers of two n = 2^L, L = 5 .. 12: fused_two_transforms (fused_rows.hip.h) with this policy ------------------
struct HilbertFused {
    using Out = cpx<float>;
    template <int N>
    static __device__ __forceinline__ void point(cpx<float> &v, const int hi, const int tau)
    {
        if (hi >= N / 2) {
            // n/2 itself (tau == 0 of the register whose other bits are zero): conj only; above it Complex32::zero(), conj'ed
            const bool half = hi == N / 2 && tau == 0;
            v = half ? mk<float>(v.re, -v.im) : mk<float>(0.0f, -0.0f);
        } else {
            const bool dc = hi == 0 && tau == 0;
            const float re2 = v.re * 2.0f, im2 = v.im * 2.0f;  // hilbert.rs:29-30
            v = dc ? mk<float>(v.re, -v.im) : mk<float>(re2, -im2);  // then ifft's conj (fft.rs:1163-1165)
        }
    }
    static __device__ __forceinline__ void store(const cpx<float> v, const float scale, const rsrc_t d, const int lane_bytes, const int off)
    {
        const float im = -v.im;
        buf_store_cpx<float>(mk<float>(v.re * scale, im * scale), d, lane_bytes, off);
    }
};

template <int L>
__global__ __launch_bounds__(256) void hilbert_fused_kernel(const float *__restrict__ x, cpx<float> *__restrict__ out,
                                                            const cpx<float> *__restrict__ tw, const size_t batch, const float scale)
{
    fused_two_transforms<L, HilbertFused>(x, out, tw, batch, scale);
}

}  // namespace host
}  // namespace kofft
