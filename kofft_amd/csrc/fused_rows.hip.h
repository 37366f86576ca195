// fused_rows.hip.h -- two n-point transforms of a row in one kernel, n = 2^L for L = 5 .. 12: what the fused routes of the Hilbert,
// cepstrum, convolve and filter-bank families share.  The register-pass machinery of fft_wg.hip.h (WgGeom, wg_compute, wg_exchange,
// lds_pad) with rl_for's geometry: a row (a frame, an item) lives in the registers of TPT threads, the forward transform runs, the
// family's pointwise step works on the last pass's registers -- whose bins the geometry names at compile time up to the thread's low
// bits --, one LDS exchange puts them back into pass-0 input order (fused_reorder) and the same forward transform runs again.
//  * FusedGeom, fused_forward, fused_reorder: the pieces, for kernels that keep a body of their own (convolve_impl.hip.h,
//    convolve_bank_impl.hip.h) and their launcher, launch_fused_items;
//  * fused_two_transforms<L, P>: the whole body for whole rows in, whole rows out, with the pointwise step and the store as a policy
//    (hilbert_impl.hip.h, cepstrum_impl.hip.h), and its host side: fused_ok, launch_fused, fused_dev;
//  * expand_real_kernel: rows of reals to rows of (x, +0), the first step of the families' composed routes.
#pragma once

#include "host_common.hip.h"

#include <type_traits>

namespace kofft {
namespace host {

// A flat grid over a whole batch (rows back to back): short rows leave no thread idle, and the grid strides over batches larger than
// it.  (static: more than one translation unit includes this header.)
static __global__ __launch_bounds__(256) void expand_real_kernel(const float *__restrict__ x, cpx<float> *__restrict__ z, const size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) st_stream(z + i, mk<float>(x[i], 0.0f));
}

// fft_wg_kernel's geometry for a stand-alone transform of this size (rl_for, 256-thread workgroups): TPT = n >> RL threads per
// row, XPB = 256 / TPT rows per workgroup, each row's exchange slot lds_elems(n) padded cells.
template <int L>
struct FusedGeom {
    static constexpr int N = 1 << L, RL = rl_for(L), R = 1 << RL, TPT = N >> RL, BLOCK = 256, XPB = BLOCK / TPT;
    static constexpr int NP = (L + RL - 1) / RL;
    static_assert(TPT <= BLOCK && BLOCK % TPT == 0 && NP >= 2 && NP <= 4, "geometry");
    static constexpr size_t lds_bytes() { return (size_t)XPB * lds_elems(N) * sizeof(cpx<float>); }
};

// The n-point forward transform (fft.rs:790-911) on registers in pass-0 input order; returns them in the last pass's output order.
template <int L>
__device__ __forceinline__ void fused_forward(cpx<float> *v, char *smem, const cpx<float> *__restrict__ tw, const int tau, const int slot)
{
    using Geo = FusedGeom<L>;
    constexpr int RL = Geo::RL, NP = Geo::NP, XPB = Geo::XPB;
    const PlainTw plain{};
    wg_compute<float, L, RL, 0>(v, plain, tw, 0, tau);
    wg_exchange<float, L, RL, 0, false, false, XPB>(v, smem, tau, slot);
    wg_compute<float, L, RL, 1>(v, plain, tw, 0, tau);
    if constexpr (NP > 2) { wg_exchange<float, L, RL, 1, false, false, XPB>(v, smem, tau, slot); wg_compute<float, L, RL, 2>(v, plain, tw, 0, tau); }
    if constexpr (NP > 3) { wg_exchange<float, L, RL, 2, false, false, XPB>(v, smem, tau, slot); wg_compute<float, L, RL, 3>(v, plain, tw, 0, tau); }
}

// Between the two transforms: the last pass's output order -> pass 0's input order, through the row's exchange slot.  Every thread of
// the workgroup comes here (three barriers).
template <int L>
__device__ __forceinline__ void fused_reorder(cpx<float> *v, char *smem, const int tau, const int slot)
{
    using Geo = FusedGeom<L>;
    constexpr int N = Geo::N, R = Geo::R;
    using G0 = WgGeom<L, Geo::RL, 0>;
    using GL = WgGeom<L, Geo::RL, Geo::NP - 1>;
    cpx<float> *buf = reinterpret_cast<cpx<float> *>(smem) + (size_t)slot * lds_elems(N);
    __syncthreads();  // every gather of the previous transform's last exchange is done
#pragma unroll
    for (int u = 0; u < R; ++u) buf[lds_pad(GL::out_index(tau, u))] = v[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < R; ++u) v[u] = buf[lds_pad(G0::in_index(tau, u))];
    __syncthreads();  // (the second transform's first exchange scatters into the same cells)
}

// The fused kernels' shared body (hilbert_fused_kernel, cepstrum_fused_kernel): rows of n = 2^L reals in, rows of P::Out out.  The
// policy P supplies
//   P::Out                                  the output element, one per point;
//   P::point<N>(v, hi, tau)                 the pointwise step, in place, on the first transform's bin hi | tau (hi =
//                                           GL::out_index(0, u), a compile-time value once unrolled), ifft's conj included;
//   P::store(v, scale, d, lane_bytes, off)  ifft's conj and * scale (fft.rs:1168-1172) on the second transform's bin, and the
//                                           store.
// (No __restrict__ here or on any helper above: the kernels' own parameters carry it.  Restrict-qualified parameters on an inlined
// body change the compiler's schedule and register counts.)
template <int L, class P>
__device__ __forceinline__ void fused_two_transforms(const float *x, typename P::Out *out, const cpx<float> *tw, const size_t batch,
                                                     const float scale)
{
    using Geo = FusedGeom<L>;
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
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    // Register u of thread tau holds bin out_index(0, u) | tau: its top bits are a compile-time fact.
#pragma unroll
    for (int u = 0; u < R; ++u) P::template point<N>(v[u], GL::out_index(0, u), tau);
    fused_reorder<L>(v, smem_raw, tau, slot);
    fused_forward<L>(v, smem_raw, tw, tau, slot);
    // bin out_index(0, u) | tau of the row
    using Out = typename P::Out;
    const rsrc_t d = make_rsrc(out + row0 * N, (unsigned)(cnt * N * sizeof(Out)));
    const int lane_bytes = (slot * N + tau) * (int)sizeof(Out);
#pragma unroll
    for (int u = 0; u < R; ++u) P::store(v[u], scale, d, lane_bytes, GL::out_index(0, u) * (int)sizeof(Out));
}

// `items` rows (frames, items) over the FusedGeom<L>::XPB slots of each 256-thread workgroup: kern(args..., scale), scale = 1 / n
// (fft.rs:1167).
template <int L, class Kernel, class... Args>
int launch_fused_items(kofft_hip_ctx *ctx, Kernel kern, size_t items, Args... args)
{
    using Geo = FusedGeom<L>;
    constexpr size_t lds = Geo::lds_bytes();
    static_assert(lds <= 64 * 1024, "LDS budget");
    const size_t blocks = (items + Geo::XPB - 1) / Geo::XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    const float scale = 1.0f / (float)Geo::N;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Geo::BLOCK), lds, ctx->stream, args..., scale);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
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
    return launch_fused_items<L>(ctx, kern, batch, d_in, reinterpret_cast<typename P::Out *>(d_out), tw, batch);
}

// The fused route of policy P for n = 32 .. 4096 (fused_ok): kernel_of(std::integral_constant<int, L>{}) is P's __global__ entry
// point for n = 2^L.
template <class P, class KernelOf>
int fused_dev(kofft_hip_ctx *ctx, KernelOf kernel_of, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const cpx<float> *tw = nullptr;
    const int rc = twiddle_table<float>(ctx, n, &tw);  // get_twiddles(n), the table of the n-point transform
    if (rc) return rc;
    return dispatch_log2<5, 12>(ilog2(n), [&](auto l) { return launch_fused<decltype(l)::value, P>(ctx, kernel_of(l), d_in, d_out, tw, batch); });
}

}  // namespace host
}  // namespace kofft
