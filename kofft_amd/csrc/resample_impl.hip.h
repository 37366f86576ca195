// resample_impl.hip.h -- polyphase resampling of float rows: upfirdn's sum, bit for bit the definition of
// include/kofft_hip.h.  Output m of a row sits at up-sampled time t = t0 + m * down, p = t mod up, i0 = t div up, and
//   out[m] = (((+0 + h[p] * x[i0]) + h[p + up] * x[i0 - 1]) + ...)      ascending j, one accumulator, product and sum un-fused
// over the terms whose sample exists (0 <= i0 - j < nx); the others are skipped, not multiplied by zero.  The translation unit is built
// with -ffp-contract=off.  Two kernels, the same operations per output:
//  * PLAIN (every shape): resample_plain_kernel, one thread per output over a flat grid, samples and taps from global memory, all
//    positions 64-bit.
//  * TILED (the footprint of resample_plan.h inside the LDS budget): resample_tiled_kernel.  A workgroup stages the taps once, phase
//    major (hp[p][j] = h[p + j * up], rows of an odd stride), then walks tiles of up to kResampleTile consecutive outputs of one row: the
//    samples the tile's terms name go into LDS with coalesced loads (only those inside [0, nx) of that row are fetched), every thread
//    sums its outputs dm = tid, tid + 256, .. out of LDS, and the stores are contiguous over the lanes.  Positions inside a tile are
//    32-bit offsets from the tile's first time, which is 64-bit.  Where the phases repeat within the workgroup (resample_phase_lanes)
//    a second instance gives a thread four outputs of one phase and reads every tap once for the four; its tiles are 4 * lanes outputs.
#pragma once

#include "host_common.hip.h"
#include "resample_plan.h"

namespace kofft {

struct ResampleShape {
    size_t nx, nh, up, down, t0, out_len;
    size_t terms;          // J
    size_t tap_stride;     // floats per phase of the tap table in LDS
    size_t tile;           // tiled kernel: outputs per tile (resample_tile_outputs)
    size_t lanes;          // tiled kernel: the threads that own outputs in the shared-phase instance (resample_phase_lanes)
    size_t tiles_per_row;
    size_t ntiles;         // rows * tiles_per_row
    size_t total;          // rows * out_len
};

__global__ __launch_bounds__(256) void resample_plain_kernel(const float *__restrict__ x, const float *__restrict__ h, float *__restrict__ out,
                                                             const ResampleShape s)
{
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < s.total; idx += (size_t)gridDim.x * 256) {
        const size_t row = idx / s.out_len, m = idx - row * s.out_len;
        const size_t t = s.t0 + m * s.down, i0 = t / s.up, p = t - i0 * s.up;
        unsigned long long jlo, jhi;
        host::resample_term_range(i0, s.nx, host::resample_terms<unsigned long long>(s.nh, s.up, p), &jlo, &jhi);
        const float *xr = x + row * s.nx;
        float acc = 0.0f;
        for (size_t j = jlo; j < jhi; ++j) {
            const float prod = h[p + j * s.up] * xr[i0 - j];
            acc = acc + prod;
        }
        out[idx] = acc;
    }
}

// the terms j in [lo, hi) of one output, ascending, onto its accumulator
__device__ __forceinline__ float resample_sum(float acc, const float *taps, const float *newest, unsigned lo, unsigned hi)
{
    for (unsigned j = lo; j < hi; ++j) {
        const float prod = taps[j] * newest[-(int)j];
        acc = acc + prod;
    }
    return acc;
}

// K outputs of one phase per thread: dm = tid, tid + lanes, .., tid + lanes (K - 1) of a tile of n outputs, K = ceil(n / lanes) the same
// for the whole workgroup, their newest samples `step` apart.  Every tap is read once for the K outputs (K + 1 LDS reads per K terms
// instead of 2 K).  Every output still adds its own terms in ascending j: the terms below the K outputs' common range first, the
// common range, the rest.  A thread whose last output lies past the tile sums its first output twice and stores it once.
template <int K>
__device__ __forceinline__ void resample_same_phase_outputs(const float *taps, const float *newest, float *orow, unsigned tid, unsigned n,
                                                            unsigned lanes, unsigned step, unsigned cnt, unsigned long long i0, unsigned long long nx)
{
    unsigned off[K], lo[K], hi[K], jl = 0, jh = cnt;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        off[k] = tid + lanes * k < n ? k * step : 0;
        unsigned long long a, b;
        host::resample_term_range(i0 + off[k], nx, cnt, &a, &b);
        lo[k] = (unsigned)a;
        hi[k] = (unsigned)b;
        jl = lo[k] > jl ? lo[k] : jl;
        jh = hi[k] < jh ? hi[k] : jh;
        acc[k] = 0.0f;
    }
    if (jl < jh) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = resample_sum(acc[k], taps, newest + off[k], lo[k], jl);
        for (unsigned j = jl; j < jh; ++j) {
            const float tap = taps[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float prod = tap * newest[(int)off[k] - (int)j];
                acc[k] = acc[k] + prod;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = resample_sum(acc[k], taps, newest + off[k], jh, hi[k]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = resample_sum(acc[k], taps, newest + off[k], lo[k], hi[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (tid + lanes * k < n) orow[tid + lanes * k] = acc[k];
}

// SAME: s.lanes * down is a multiple of up (resample_phase_lanes), so the outputs tid, tid + lanes, tid + 2 lanes, tid + 3 lanes of a
// tile of 4 lanes outputs share their phase and resample_same_phase_outputs sums them together; the threads from `lanes` on only stage.
template <bool SAME>
__global__ __launch_bounds__(256) void resample_tiled_kernel(const float *__restrict__ x, const float *__restrict__ h, float *__restrict__ out,
                                                             const ResampleShape s)
{
    extern __shared__ float resample_lds[];
    float *hp = resample_lds;
    float *xs = resample_lds + s.up * s.tap_stride;
    const unsigned tid = threadIdx.x, up = (unsigned)s.up, down = (unsigned)s.down, J = (unsigned)s.terms, stride = (unsigned)s.tap_stride;
    const unsigned nh = (unsigned)s.nh;
    for (unsigned n = tid; n < nh; n += 256) {  // (nh <= up * J inside the budget: 32 bits)
        const unsigned j = n / up, p = n - j * up;
        hp[p * stride + j] = h[n];
    }
    const unsigned tile_outputs = SAME ? (unsigned)s.tile : host::kResampleTile;  // (s.tile either way; a constant where it can be)
    for (size_t tile = blockIdx.x; tile < s.ntiles; tile += gridDim.x) {
        const size_t row = tile / s.tiles_per_row, m0 = (tile - row * s.tiles_per_row) * tile_outputs;
        const size_t left = s.out_len - m0;
        const unsigned n = left < tile_outputs ? (unsigned)left : tile_outputs;
        const host::ResampleTile tl = host::resample_tile(s.t0, m0, n, s.up, s.down, J);
        const float *xr = x + row * s.nx;
        __syncthreads();  // the tile before this one has been read
        for (unsigned k = tid; k < (unsigned)tl.s_count; k += 256) {
            const long long i = tl.s_first + (long long)k;
            xs[k] = (i >= 0 && (unsigned long long)i < s.nx) ? xr[i] : 0.0f;
        }
        __syncthreads();  // (the first time: the taps too)
        float *orow = out + row * s.out_len + m0;
        if (SAME) {
            const unsigned lanes = (unsigned)s.lanes;
            if (tid < lanes && tid < n) {
                unsigned p, di;
                host::resample_output(tl.r_first, tid, up, down, &p, &di);
                const unsigned cnt = host::resample_terms<unsigned>(nh, up, p), step = lanes * down / up;
                const float *taps = hp + p * stride;
                const float *newest = xs + di + (J - 1);
                switch ((n + lanes - 1) / lanes) {  // (the same for every thread of the workgroup)
                case 1: resample_same_phase_outputs<1>(taps, newest, orow, tid, n, lanes, step, cnt, tl.q_first + di, s.nx); break;
                case 2: resample_same_phase_outputs<2>(taps, newest, orow, tid, n, lanes, step, cnt, tl.q_first + di, s.nx); break;
                case 3: resample_same_phase_outputs<3>(taps, newest, orow, tid, n, lanes, step, cnt, tl.q_first + di, s.nx); break;
                default: resample_same_phase_outputs<4>(taps, newest, orow, tid, n, lanes, step, cnt, tl.q_first + di, s.nx); break;
                }
            }
            continue;
        }
        for (unsigned dm = tid; dm < n; dm += 256) {
            unsigned p, di;
            host::resample_output(tl.r_first, dm, up, down, &p, &di);
            unsigned long long jlo, jhi;
            host::resample_term_range(tl.q_first + di, s.nx, host::resample_terms<unsigned>(nh, up, p), &jlo, &jhi);
            orow[dm] = resample_sum(0.0f, hp + p * stride, xs + di + (J - 1), (unsigned)jlo, (unsigned)jhi);
        }
    }
}

}  // namespace kofft
