// hilbert_impl.hip.h -- hilbert::hilbert_analytic (hilbert.rs:13-47) on device pointers, f32 only like the reference.
//
// For a row of n reals (n a power of two; anything else is the reference's NonPowerOfTwoNoStd) the reference computes
//   freq = fft((x, +0));  bins 1 .. n/2-1: re *= 2, im *= 2;  bins n/2+1 .. n-1 = (+0, +0);  out = ifft(freq)
// with ifft = conj (im = -im), fft, conj, * (1 / n) and an early return at n == 1 (fft.rs:1134-1174).  The mask is two real
// multiplies (an Inf stays an Inf; a complex multiply by (2, 0) would make NaNs), and the conj is a negation, so a zeroed bin
// enters the second transform as (+0, -0).  Two routes, the same operations per element:
//  * fused (powers of two n = 32 .. 4096): hilbert_fused_kernel<L>, one pass over HBM, whose body (fused_two_transforms) the
//    cepstrum's fused kernel shares.  The register-pass machinery of fft_wg.hip.h (WgGeom, reg_pass, wg_exchange, lds_pad) with
//    rl_for's geometry: rows load as (x, +0) through one buffer descriptor per workgroup, the forward transform runs, the last
//    pass's registers -- whose bins the geometry names at compile time up to the thread's low bits -- take mask + conj, one LDS
//    exchange puts them back into pass-0 input order, the same forward transform runs again and the store applies conj * scale;
//  * composed (n <= 16, whose transforms are the reference's straight-line kernels, powers of two above 4096, inputs that are not
//    4-byte aligned, and every n after kofft_hip_set_hilbert_fused(ctx, 0)): the caller's output is the workspace --
//    hilbert_expand_kernel writes (x, +0), fft_dev transforms in place, hilbert_mask_kernel masks, fft_dev(inverse) runs the
//    reference's ifft in place.
#pragma once

#include "host_common.hip.h"

#include <type_traits>

namespace kofft {
namespace host {

// ---- composed route ---------------------------------------------------------------------------------------------------------
// Flat grids over the whole batch (rows back to back; n is a power of two, so a sample's bin is its index's low bits): short rows
// leave no thread idle, and the grid strides over batches larger than it.  (static: k_hilbert_f32.hip and k_convolve_f32.hip both
// include this header.)
static __global__ __launch_bounds__(256) void hilbert_expand_kernel(const float *__restrict__ x, cpx<float> *__restrict__ z, const size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) st_stream(z + i, mk<float>(x[i], 0.0f));
}

// hilbert.rs:28-34 (n even, n >= 4): bins 0 and n/2 untouched, 1 .. n/2-1 doubled part by part, n/2+1 .. n-1 = Complex32::zero()
static __global__ __launch_bounds__(256) void hilbert_mask_kernel(cpx<float> *__restrict__ z, const size_t n, const size_t total)
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

inline unsigned hilbert_flat_blocks(const kofft_hip_ctx *ctx, size_t total)
{
    const size_t want = (total + 255) / 256, cap = (size_t)ctx->num_cus * 64;
    return (unsigned)(want < cap ? want : cap);
}

inline int hilbert_composed_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    cpx<float> *z = reinterpret_cast<cpx<float> *>(d_out);
    const size_t total = n * batch;
    hipLaunchKernelGGL(hilbert_expand_kernel, dim3(hilbert_flat_blocks(ctx, total)), dim3(256), 0, ctx->stream, d_in, z, total);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    if (n == 1) return KOFFT_OK;  // fft: nothing (fft.rs:1059); n odd: no mask; ifft returns early (fft.rs:1139)
    int rc = fft_dev<float>(ctx, d_out, d_out, n, batch, 0);  // hilbert.rs:25
    if (rc) return rc;
    if (n > 2) {  // (n = 2: bins 1 .. 0 and 2 .. 1 -- nothing to mask)
        hipLaunchKernelGGL(hilbert_mask_kernel, dim3(hilbert_flat_blocks(ctx, total)), dim3(256), 0, ctx->stream, z, n, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return fft_dev<float>(ctx, d_out, d_out, n, batch, 1);  // hilbert.rs:45: conj, fft, conj * (1 / n)
}

// ---- fused route: powers of two n = 2^L, L = 5 .. 12 ------------------------------------------------------------------------
// fft_wg_kernel's geometry for a stand-alone transform of this size (rl_for, 256-thread workgroups): TPT = n >> RL threads per
// row, XPB = 256 / TPT rows per workgroup, each row's exchange slot lds_elems(n) padded cells.
template <int L>
struct HilbertGeom {
    static constexpr int N = 1 << L, RL = rl_for(L), R = 1 << RL, TPT = N >> RL, BLOCK = 256, XPB = BLOCK / TPT;
    static constexpr int NP = (L + RL - 1) / RL;
    static_assert(TPT <= BLOCK && BLOCK % TPT == 0 && NP >= 2 && NP <= 4, "geometry");
    static constexpr size_t lds_bytes() { return (size_t)XPB * lds_elems(N) * sizeof(cpx<float>); }
};

// The n-point forward transform (fft.rs:790-911) on registers in pass-0 input order; returns them in the last pass's output order.
template <int L>
__device__ __forceinline__ void hilbert_forward(cpx<float> *v, char *smem, const cpx<float> *__restrict__ tw, const int tau, const int slot)
{
    using Geo = HilbertGeom<L>;
    constexpr int RL = Geo::RL, NP = Geo::NP, XPB = Geo::XPB;
    const PlainTw plain{};
    wg_compute<float, L, RL, 0>(v, plain, tw, 0, tau);
    wg_exchange<float, L, RL, 0, false, false, XPB>(v, smem, tau, slot);
    wg_compute<float, L, RL, 1>(v, plain, tw, 0, tau);
    if constexpr (NP > 2) { wg_exchange<float, L, RL, 1, false, false, XPB>(v, smem, tau, slot); wg_compute<float, L, RL, 2>(v, plain, tw, 0, tau); }
    if constexpr (NP > 3) { wg_exchange<float, L, RL, 2, false, false, XPB>(v, smem, tau, slot); wg_compute<float, L, RL, 3>(v, plain, tw, 0, tau); }
}

// The fused kernels' shared body (hilbert_fused_kernel, cepstrum_fused_kernel): rows of n = 2^L reals in, rows of P::Out out.  The
// policy P supplies
//   P::Out                                  the output element, one per point;
//   P::point<N>(v, hi, tau)                 the pointwise step, in place, on the first transform's bin hi | tau (hi =
//                                           GL::out_index(0, u), a compile-time value once unrolled), ifft's conj included;
//   P::store(v, scale, d, lane_bytes, off)  ifft's conj and * scale (fft.rs:1168-1172) on the second transform's bin, and the
//                                           store.
// (No __restrict__ here: the kernels' own parameters carry it.  Restrict-qualified parameters on this inlined body change the
// compiler's schedule and register counts.)
template <int L, class P>
__device__ __forceinline__ void fused_two_transforms(const float *x, typename P::Out *out, const cpx<float> *tw, const size_t batch,
                                                     const float scale)
{
    using Geo = HilbertGeom<L>;
    constexpr int N = Geo::N, R = Geo::R, TPT = Geo::TPT, XPB = Geo::XPB;
    using G0 = WgGeom<L, Geo::RL, 0>;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, tau = tid % TPT, slot = tid / TPT;
    const size_t row0 = (size_t)blockIdx.x * XPB;  // < batch (grid = ceil(batch / XPB))
    const size_t cnt = batch - row0 < (size_t)XPB ? batch - row0 : (size_t)XPB;
    // One descriptor over the workgroup's rows, cut at the end of the batch: the rows past it read zeros and store nothing, with no
    // per-lane test.  Pass 0's register u of thread tau holds sample in_index(0, u) + tau of its row.
    cpx<float> v[R];
    {
        const rsrc_t d = make_rsrc(x + row0 * N, (unsigned)(cnt * N * sizeof(float)));
        const int lane_bytes = (slot * N + tau) * (int)sizeof(float);
        float raw[R];
#pragma unroll
        for (int u = 0; u < R; ++u) raw[u] = buf_load_f32<AUX_NT>(d, lane_bytes, G0::in_index(0, u) * (int)sizeof(float));
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = mk<float>(raw[u], 0.0f);  // hilbert.rs:21-23, cepstrum.rs:21-23
    }
    hilbert_forward<L>(v, smem_raw, tw, tau, slot);
    // Register u of thread tau holds bin out_index(0, u) | tau: its top bits are a compile-time fact.
#pragma unroll
    for (int u = 0; u < R; ++u) P::template point<N>(v[u], GL::out_index(0, u), tau);
    {   // last pass's output order -> pass 0's input order, through the row's exchange slot
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
    // bin out_index(0, u) | tau of the row
    using Out = typename P::Out;
    const rsrc_t d = make_rsrc(out + row0 * N, (unsigned)(cnt * N * sizeof(Out)));
    const int lane_bytes = (slot * N + tau) * (int)sizeof(Out);
#pragma unroll
    for (int u = 0; u < R; ++u) P::store(v[u], scale, d, lane_bytes, GL::out_index(0, u) * (int)sizeof(Out));
}

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

// (the kernels' loads are 4 bytes wide: an input that is not 4-byte aligned takes the composed route; `enabled` is the context's
// switch, kofft_hip_set_hilbert_fused / kofft_hip_set_cepstrum_fused)
inline bool fused_ok(const bool enabled, const float *d_in, size_t n)
{
    return enabled && n >= 32 && n <= 4096 && (reinterpret_cast<size_t>(d_in) & 3) == 0;
}

template <int L, class P, class Kernel>
int launch_fused(kofft_hip_ctx *ctx, Kernel kern, const float *d_in, float *d_out, const cpx<float> *tw, size_t batch)
{
    using Geo = HilbertGeom<L>;
    constexpr size_t lds = Geo::lds_bytes();
    static_assert(lds <= 64 * 1024, "LDS budget");
    const size_t blocks = (batch + Geo::XPB - 1) / Geo::XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    const float scale = 1.0f / (float)Geo::N;  // fft.rs:1167
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Geo::BLOCK), lds, ctx->stream, d_in,
                       reinterpret_cast<typename P::Out *>(d_out), tw, batch, scale);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// The fused route of policy P for n = 32 .. 4096 (fused_ok): kernel_of(std::integral_constant<int, L>{}) is P's __global__ entry
// point for n = 2^L.
template <class P, class KernelOf>
int fused_dev(kofft_hip_ctx *ctx, KernelOf kernel_of, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const cpx<float> *tw = nullptr;
    const int rc = twiddle_table<float>(ctx, n, &tw);  // get_twiddles(n), the table of the n-point transform
    if (rc) return rc;
    using std::integral_constant;
    switch (ilog2(n)) {
    case 5: return launch_fused<5, P>(ctx, kernel_of(integral_constant<int, 5>{}), d_in, d_out, tw, batch);
    case 6: return launch_fused<6, P>(ctx, kernel_of(integral_constant<int, 6>{}), d_in, d_out, tw, batch);
    case 7: return launch_fused<7, P>(ctx, kernel_of(integral_constant<int, 7>{}), d_in, d_out, tw, batch);
    case 8: return launch_fused<8, P>(ctx, kernel_of(integral_constant<int, 8>{}), d_in, d_out, tw, batch);
    case 9: return launch_fused<9, P>(ctx, kernel_of(integral_constant<int, 9>{}), d_in, d_out, tw, batch);
    case 10: return launch_fused<10, P>(ctx, kernel_of(integral_constant<int, 10>{}), d_in, d_out, tw, batch);
    case 11: return launch_fused<11, P>(ctx, kernel_of(integral_constant<int, 11>{}), d_in, d_out, tw, batch);
    case 12: return launch_fused<12, P>(ctx, kernel_of(integral_constant<int, 12>{}), d_in, d_out, tw, batch);
    default: return KOFFT_ERR_UNSUPPORTED;  // (never: fused_ok)
    }
}

}  // namespace host
}  // namespace kofft
