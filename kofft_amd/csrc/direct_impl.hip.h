// direct_impl.hip.h -- dct::dct1..dct4 (dct.rs:108-176) and dst::dst1..dst4 (dst.rs:89-146) on device pointers, f32 only like
// the reference.
//
// Every one of the eight transforms is out[b][k] = init(x[b]) + sum_i x'[b][i] * C[i][k], summed in increasing i, one f32
// multiply and one f32 add per term (-ffp-contract=off: never fused).  C depends on the kind and n only: it is built on the
// host (tables.cpp: the reference's angle, then glibc cosf / sinf) and cached per (context, kind, n) in the context's table
// cache, with its row stride padded to a multiple of DT_BN floats (the padding is zero).  x' = 2 * x for DCT-I (dct.rs:126:
// `2.0 * x * cos`), x otherwise.  init: DCT-I x0 + x[n-1] (k even) or x0 + (-x[n-1]) (k odd), and [2 * x0] at n = 1 (dct.rs:
// 110-124); DCT-III and DST-III x0 / 2.0 (dct.rs:153, dst.rs:123); the rest +0.0.  The accumulator is SEEDED with init before
// the first term: f32 addition is not associative, so any other order changes bits.
// Two kernels, the same operations per output:
//  * direct_tiled_kernel<M>: a workgroup owns DT_BM rows x DT_BN outputs k; it walks i in chunks of DT_KC, stages x'[rows][chunk]
//    and C[chunk][k-tile] in LDS (the global loads of chunk c + 1 are issued before chunk c is computed) and every lane updates an
//    8 x 8 register tile with packed multiplies and packed adds (v_pk_mul_f32, v_pk_add_f32);
//  * direct_simple_kernel<M>: one lane per (row, k), C[i][k] read from global memory; small n and small batches (direct_use_tiled),
//    and every call of a context after kofft_hip_set_direct_tiled(ctx, 0).
#pragma once

#include "host_common.hip.h"

namespace kofft {
namespace host {

enum DirectInit { DIR_ZERO = 0, DIR_HALF = 1, DIR_DCT1 = 2 };

// init(x[b]) at output k (see the top of the file); xr is the row, read only by the modes that need it
template <int M>
__device__ __forceinline__ float direct_init(const float *__restrict__ xr, int n, int k)
{
    if constexpr (M == DIR_ZERO) {
        return 0.0f;
    } else if constexpr (M == DIR_HALF) {
        return xr[0] / 2.0f;
    } else {
        if (n == 1) return xr[0] * 2.0f;  // dct.rs:113-115
        const float last = xr[n - 1];
        return xr[0] + ((k & 1) ? -last : last);
    }
}

template <int M>
__device__ __forceinline__ float direct_term_x(float v)
{
    if constexpr (M == DIR_DCT1) return 2.0f * v;
    else return v;
}

// ---- simple kernel: one lane per (row, k) ---------------------------------------------------------------------------------------
// A row holds n inputs and nk outputs (the eight DCT / DST kinds: nk = n; the chirp-Z sums of spectral_impl.hip.h: nk = 2 m, the
// interleaved complex bins).  A workgroup covers rpb = 256 / nk rows (nk < 256: lane = row * nk + k, one 32-bit division) or 256
// outputs k of one row (blockIdx.x walks the k chunks); blockIdx.y strides over the row groups.  (No 64-bit division: its expansion
// holds v_fmac_f32.)
template <int M>
__global__ __launch_bounds__(256) void direct_simple_kernel(const float *__restrict__ x, const float *__restrict__ c, float *__restrict__ out,
                                                            const int n, const int nk, const int ldc, const int ib, const int ie,
                                                            const size_t batch, const int rpb)
{
    const unsigned tid = threadIdx.x;
    unsigned r = 0, k = blockIdx.x * 256u + tid;
    if (rpb > 1) {
        r = tid / (unsigned)nk;
        k = tid - r * (unsigned)nk;
        if (r >= (unsigned)rpb) return;
    }
    if (k >= (unsigned)nk) return;
    const float *ck = c + k;
    for (size_t b = (size_t)blockIdx.y * rpb + r; b < batch; b += (size_t)gridDim.y * rpb) {
        const float *xr = x + b * n;
        float acc = direct_init<M>(xr, n, (int)k);
        for (int i = ib; i < ie; ++i) acc = acc + direct_term_x<M>(xr[i]) * ck[(size_t)i * ldc];
        out[b * nk + k] = acc;
    }
}

// ---- tiled kernel -----------------------------------------------------------------------------------------------------------------
// 256 lanes as 16 (tx, along k) x 16 (ty, along rows).  Lane (tx, ty) owns rows {4ty .. 4ty+3, 64+4ty .. 64+4ty+3} and outputs
// {4tx .. 4tx+3, 64+4tx .. 64+4tx+3} of the tile: each of its four ds_read_b128 per i reads 16 consecutive bytes per lane and 256
// consecutive bytes per 16 lanes (no bank conflict), and its stores are 16 consecutive bytes per lane.
constexpr int DT_BM = 128, DT_BN = 128, DT_KC = 16;
constexpr int DT_XS = DT_BM + 4;  // Xs row stride: the transposing b32 writes hit 8 banks instead of 1, rows stay 16-byte aligned

typedef float dt_f2 __attribute__((ext_vector_type(2)));
typedef float dt_f4 __attribute__((ext_vector_type(4)));

template <int M>
__global__ __launch_bounds__(256) void direct_tiled_kernel(const float *__restrict__ x, const float *__restrict__ c, float *__restrict__ out,
                                                           const int n, const int nk, const int ldc, const int ib, const int ie,
                                                           const size_t batch, const unsigned ktiles, const bool vec_out)
{
    __shared__ __attribute__((aligned(16))) float xs[DT_KC][DT_XS];
    __shared__ __attribute__((aligned(16))) float cs[DT_KC][DT_BN];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int k0 = (int)(blockIdx.x % ktiles) * DT_BN;  // neighbouring workgroups share a row tile (its x is read from L2 once)
    const size_t row0 = (size_t)(blockIdx.x / ktiles) * DT_BM;

    // staging roles: x -- lane (li = tid & 15, lr = tid >> 4) loads rows lr + 16 j of i = i0 + li (consecutive lanes: consecutive
    // i of one row); C -- float4 q = tid + 256 j of the chunk, i = i0 + q / 32, k = k0 + 4 (q % 32) (the table's rows are padded
    // to a multiple of DT_BN floats: no k bound)
    const int li = tid & 15, lr = tid >> 4;
    float xv[8];
    dt_f4 cv[2];
    auto load = [&](int i0) {
        const int i = i0 + li;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t row = row0 + lr + 16 * j;
            xv[j] = (i < ie && row < batch) ? direct_term_x<M>(x[row * n + i]) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = tid + 256 * j, ic = i0 + (q >> 5);
            cv[j] = ic < ie ? *reinterpret_cast<const dt_f4 *>(c + (size_t)ic * ldc + k0 + 4 * (q & 31)) : dt_f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) xs[li][lr + 16 * j] = xv[j];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = tid + 256 * j;
            *reinterpret_cast<dt_f4 *>(&cs[q >> 5][4 * (q & 31)]) = cv[j];
        }
    };

    // the accumulators, seeded with init: acc[r][p] holds outputs (kc(p), kc(p) + 1) of row rr(r)
    auto rr = [&](int r) { return (r < 4 ? 0 : 64 - 4) + 4 * ty + r; };
    auto kc = [&](int p) { return (p < 2 ? 0 : 64 - 4) + 4 * tx + 2 * p; };
    dt_f2 acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const size_t row = row0 + rr(r);
        const float *xr = x + (row < batch ? row : 0) * n;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int k = k0 + kc(p);
            acc[r][p].x = direct_init<M>(xr, n, k);
            acc[r][p].y = direct_init<M>(xr, n, k + 1);
        }
    }

    auto step = [&](int ii) {
        const dt_f4 xa = *reinterpret_cast<const dt_f4 *>(&xs[ii][4 * ty]);
        const dt_f4 xb = *reinterpret_cast<const dt_f4 *>(&xs[ii][64 + 4 * ty]);
        const dt_f4 ca = *reinterpret_cast<const dt_f4 *>(&cs[ii][4 * tx]);
        const dt_f4 cb = *reinterpret_cast<const dt_f4 *>(&cs[ii][64 + 4 * tx]);
        const float xr[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        const dt_f2 cp[4] = {dt_f2{ca.x, ca.y}, dt_f2{ca.z, ca.w}, dt_f2{cb.x, cb.y}, dt_f2{cb.z, cb.w}};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const dt_f2 xx = dt_f2{xr[r], xr[r]};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const dt_f2 t = xx * cp[p];  // one rounding: the term
                acc[r][p] = acc[r][p] + t;   // one rounding: the sum
            }
        }
    };

    if (ib < ie) load(ib);
    for (int i0 = ib; i0 < ie; i0 += DT_KC) {
        stage();
        __syncthreads();
        if (i0 + DT_KC < ie) load(i0 + DT_KC);  // in flight while this chunk is computed
        const int cnt = ie - i0 < DT_KC ? ie - i0 : DT_KC;
        if (cnt == DT_KC) {
#pragma unroll
            for (int ii = 0; ii < DT_KC; ++ii) step(ii);
        } else {
            for (int ii = 0; ii < cnt; ++ii) step(ii);
        }
        __syncthreads();
    }

    // 16-byte stores (vec_out: nk % 4 == 0 and a 16-byte aligned output) through b128_store_guard, else 4-byte ones
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const size_t row = row0 + rr(r);
        if (row >= batch) continue;
        float *orow = out + row * nk;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k0 + kc(2 * h);
            const dt_f4 v = dt_f4{acc[r][2 * h].x, acc[r][2 * h].y, acc[r][2 * h + 1].x, acc[r][2 * h + 1].y};
            if (vec_out && k + 4 <= nk) {
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                const v4u bits = __builtin_bit_cast(v4u, v);
                *reinterpret_cast<v4u *>(orow + k) = bits;
                b128_store_guard(bits);
            } else {
                if (k < nk) orow[k] = v.x;
                if (k + 1 < nk) orow[k + 1] = v.y;
                if (k + 2 < nk) orow[k + 2] = v.z;
                if (k + 3 < nk) orow[k + 3] = v.w;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
inline size_t direct_ldc(size_t n) { return (n + DT_BN - 1) / DT_BN * DT_BN; }

// The n x direct_ldc(n) table of one kind, built on the host at the first call of a (context, kind, n) and kept until the context
// is destroyed (kofft_hip_destroy frees the whole cache).
inline int get_direct_table(kofft_hip_ctx *ctx, int family, int type, size_t n, const float **out)
{
    const size_t ldc = direct_ldc(n), bytes = n * ldc * sizeof(float);
    return device_table(ctx, direct_table_kind(family, type), n, bytes, "direct table upload", out, [&](void *d, std::string &why) {
        std::vector<float> host(n * ldc);
        kofft_tables::direct_table_f32(family, type, n, ldc, host.data());
        return upload_table(d, host.data(), bytes, why);
    });
}

// Where a tile would be mostly padding the simple kernel runs (the crossover measured with tools/bench_trig_direct.py);
// nk: the outputs per row
inline bool direct_use_tiled(const kofft_hip_ctx *ctx, size_t nk, size_t batch)
{
    return ctx->direct_tiled && nk >= 64 && batch >= 64;
}

template <int M>
int launch_direct(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *table, size_t n, size_t nk, size_t batch, size_t ib,
                  size_t ie)
{
    const int ldc = (int)direct_ldc(nk);
    if (direct_use_tiled(ctx, nk, batch)) {
        const unsigned ktiles = (unsigned)(ldc / DT_BN);
        const bool vec_out = (nk % 4) == 0 && (reinterpret_cast<size_t>(d_out) & 15) == 0;
        // row tiles per launch: a grid of at most 2^30 workgroups
        const size_t max_rows = (size_t(1) << 30) / ktiles * DT_BM;
        for (size_t b0 = 0; b0 < batch; b0 += max_rows) {
            const size_t nb = batch - b0 < max_rows ? batch - b0 : max_rows;
            const size_t blocks = (nb + DT_BM - 1) / DT_BM * ktiles;
            hipLaunchKernelGGL(direct_tiled_kernel<M>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_in + b0 * n, table, d_out + b0 * nk,
                               (int)n, (int)nk, ldc, (int)ib, (int)ie, nb, ktiles, vec_out);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        return KOFFT_OK;
    }
    const int rpb = nk < 256 ? (int)(256 / nk) : 1;
    const size_t groups = (batch + rpb - 1) / rpb;
    const dim3 grid((unsigned)((nk + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(direct_simple_kernel<M>, grid, dim3(256), 0, ctx->stream, d_in, table, d_out, (int)n, (int)nk, ldc, (int)ib, (int)ie, batch,
                       rpb);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft
