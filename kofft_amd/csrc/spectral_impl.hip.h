// spectral_impl.hip.h -- czt::czt_f32 (czt.rs:16-54) and goertzel::goertzel_f32 (goertzel.rs:16-36, the std form) on device
// pointers, f32 only like the reference.  Every operation is one f32 rounding in the reference's order (-ffp-contract=off: never
// fused); the device computes no trigonometry and no division.
//
// Chirp-Z.  out[b][k] = sum_i x[b][i] * C[i][k], C[i][k] = apow[i] * wnk_k[i], where apow[i] is a_inv multiplied i times into (1, 0)
// and wnk_k[i] is wpow[k] multiplied i times into (1, 0) (wpow[k]: w multiplied k times into (1, 0)).  wpow and apow are sequential
// prefixes of at most 4096 steps, built on the host (tables.cpp) and uploaded; wnk is the recurrence each lane carries:
//  * czt_recur_kernel<CZT_TABLE>: one lane per bin k walks i and writes C[i][2k], C[i][2k + 1] (one 8-byte store per lane, coalesced
//    over k) into an n x ldc table, ldc = 2 m rounded up to DT_BN floats; lanes m .. ldc / 2 - 1 write the +0 padding.  That is the
//    layout direct_tiled_kernel<DIR_ZERO> / direct_simple_kernel<DIR_ZERO> (direct_impl.hip.h) read for a row of nk = 2 m outputs, so
//    the sums run there: +0 seed, terms in increasing i, one multiply and one add each -- the bytes of the SUM mode.
//  * czt_recur_kernel<CZT_SUM>: one lane per (row, k) carries the same recurrence and accumulates against x[row][i] on the fly; no
//    table.  For batches too small to repay one (czt_use_table).
// Tables are kept per (n, m, bits of w and a), at most four per context, least recently used first out (k_spectral_f32.hip).
//
// Goertzel.  One lane owns one (row, frequency) and carries s_prev, s_prev2 and coeff in registers: s = (x + coeff * s_prev) - s_prev2
// per sample, a dependent chain of three operations.  Splitting a row across lanes would change the bits, so all the parallelism is
// rows x frequencies: a single row against a single frequency is one lane walking n samples, slow by construction.  A 256-lane
// workgroup owns rpb rows x fpb frequencies (frequency fastest across lanes) and walks the rows in chunks of GZ_GC samples staged in
// LDS: 16-byte global loads where the rows are 16-byte aligned (n % 4 == 0 and an aligned base), 4-byte ones otherwise, coalesced
// along i; the next chunk's loads are issued before the current chunk is computed (the pattern of direct_tiled_kernel).  The LDS row
// stride is GZ_GC + 1 floats: lanes of different rows read different banks, lanes of one row read one address (a broadcast).  The
// kernel ends with sqrtf of power = (s2 * s2 + s1 * s1) - (coeff * s1) * s2, the correctly rounded root stft_magnitudes uses.  The
// root is a called (not inlined) device function, spectral_root_cr: its expansion holds fused operations of its own, and as a
// function of its own it leaves goertzel_kernel's body free of them, which the machine-code test demands of the recurrence.
// coeff[nfreq] comes from the host (tables.cpp: glibc cosf); the device-pointer form brings it over in kernel arguments
// (spectral_fill_kernel), 256 values per launch, so that the call stays asynchronous and needs no host buffer that outlives it.
#pragma once

#include "direct_impl.hip.h"

namespace kofft {
namespace host {

enum CztMode { CZT_TABLE = 0, CZT_SUM = 1 };

typedef float sp_f2 __attribute__((ext_vector_type(2)));
typedef float sp_f4 __attribute__((ext_vector_type(4)));

// Lanes as in direct_simple_kernel: rpb = 256 / m rows per workgroup (m < 256: lane = row * m + k, one 32-bit division) or blockDim.x
// bins of one row (blockIdx.x walks the k chunks); blockIdx.y strides over the row groups.  TABLE: batch = 1, rpb = 1, m is the padded
// bin count ldc / 2 and m_real the bins that hold values.
template <int MODE>
__global__ __launch_bounds__(256) void czt_recur_kernel(const float *__restrict__ x, const float *__restrict__ wpow, const float *__restrict__ apow,
                                                        float *__restrict__ dst, const int n, const int m, const int m_real, const int ldc,
                                                        const size_t batch, const int rpb)
{
    const unsigned tid = threadIdx.x;
    unsigned r = 0, k = blockIdx.x * blockDim.x + tid;
    if (rpb > 1) {
        r = tid / (unsigned)m;
        k = tid - r * (unsigned)m;
        if (r >= (unsigned)rpb) return;
    }
    if (k >= (unsigned)m) return;
    const bool live = k < (unsigned)m_real;
    const sp_f2 wk = live ? *reinterpret_cast<const sp_f2 *>(wpow + 2 * k) : sp_f2{0.0f, 0.0f};
    const sp_f2 *ap = reinterpret_cast<const sp_f2 *>(apow);
    for (size_t b = (size_t)blockIdx.y * rpb + r; b < batch; b += (size_t)gridDim.y * rpb) {
        float wr = live ? 1.0f : 0.0f, wi = 0.0f;  // wnk (padding lanes: +0 throughout, 0 * anything finite; their stores are forced to +0 below)
        float accr = 0.0f, acci = 0.0f;
        const float *xr = x + b * n;
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const sp_f2 a = ap[i];
            const float tr = a.x * wr - a.y * wi;  // czt.rs:38-39
            const float ti = a.x * wi + a.y * wr;
            if constexpr (MODE == CZT_TABLE) {
                *reinterpret_cast<sp_f2 *>(dst + (size_t)i * ldc + 2 * k) = live ? sp_f2{tr, ti} : sp_f2{0.0f, 0.0f};
            } else {
                const float xv = xr[i];
                accr = accr + xv * tr;  // czt.rs:40-41
                acci = acci + xv * ti;
            }
            const float nr = wr * wk.x - wi * wk.y;  // czt.rs:43-46
            const float ni = wr * wk.y + wi * wk.x;
            wr = nr;
            wi = ni;
        }
        if constexpr (MODE == CZT_SUM) {
            float *o = dst + (b * m + k) * 2;  // 4-byte stores: the output may be 4-byte aligned only
            o[0] = accr;
            o[1] = acci;
        }
    }
}

// ---- Goertzel ------------------------------------------------------------------------------------------------------------------
// sqrtf, correctly rounded (hipcc's default for sqrtf; a negative or NaN argument gives NaN, goertzel.rs:35), kept out of line
__device__ __attribute__((noinline)) float spectral_root_cr(const float v) { return sqrtf(v); }

// dst[0 .. count) = c.v[0 .. count): the values travel in the kernel arguments
constexpr int SP_FILL = 256;
struct sp_fill_chunk {
    float v[SP_FILL];
};
__global__ __launch_bounds__(SP_FILL) void spectral_fill_kernel(float *__restrict__ dst, const sp_fill_chunk c, const int count)
{
    if ((int)threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

constexpr int GZ_GC = 32;           // samples per staged chunk
constexpr int GZ_XS = GZ_GC + 1;    // LDS row stride: odd, so the 32 lanes of a ds_read_b32 group, one row each, hit 32 banks
constexpr int GZ_ROWS = 256;        // rows of the LDS tile (nfreq = 1: one row per lane)

// fpb = min(nfreq, 256) frequencies and rpb = 256 / fpb rows per workgroup; blockIdx.x: the frequency chunk, blockIdx.y strides over
// the `groups` row groups.  vec_in: every row is 16-byte aligned (n % 4 == 0, aligned base), so a float4 never straddles the row end.
__global__ __launch_bounds__(256, 2) void goertzel_kernel(const float *__restrict__ x, const float *__restrict__ coeff, float *__restrict__ out,
                                                       const int n, const int nfreq, const size_t batch, const int fpb, const int rpb,
                                                       const size_t groups, const bool vec_in)
{
    __shared__ float xs[GZ_ROWS * GZ_XS];
    const unsigned tid = threadIdx.x;
    const unsigned r = tid / (unsigned)fpb;
    const unsigned f = blockIdx.x * (unsigned)fpb + (tid - r * (unsigned)fpb);
    const bool lane_ok = r < (unsigned)rpb && f < (unsigned)nfreq;
    const float c = lane_ok ? coeff[f] : 0.0f;
    const unsigned tile_q = (unsigned)rpb * (vec_in ? GZ_GC / 4 : GZ_GC);  // float4s / floats of one staged tile

    for (size_t g = blockIdx.y; g < groups; g += gridDim.y) {
        const size_t row0 = g * (size_t)rpb;
        float xv[GZ_GC];
        // lane tid covers tile rows (tid >> 3) + 32 j at float4 tid & 7 (vec_in) or rows (tid >> 5) + 8 j at sample tid & 31: one running
        // 64-bit address and one row count per lane instead of an address per load
        const unsigned lrow = vec_in ? tid >> 3 : tid >> 5, lcol = vec_in ? 4 * (tid & 7) : tid & 31, lstep = vec_in ? 32 : 8;
        const size_t left = batch - row0;
        const unsigned nrows = left < (size_t)rpb ? (unsigned)left : (unsigned)rpb;  // rows of this tile that exist
        auto load = [&](int i0) {
            const bool col_ok = i0 + (int)lcol < n;
            const float *p = x + (row0 + lrow) * n + i0 + lcol;
            const size_t step = (size_t)lstep * n;
            if (vec_in) {
#pragma unroll
                for (int j = 0; j < GZ_GC / 4; ++j) {
                    sp_f4 v = sp_f4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (col_ok && lrow + 32u * j < nrows) v = *reinterpret_cast<const sp_f4 *>(p);
                    p += step;
                    xv[4 * j] = v.x;
                    xv[4 * j + 1] = v.y;
                    xv[4 * j + 2] = v.z;
                    xv[4 * j + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < GZ_GC; ++j) {
                    xv[j] = (col_ok && lrow + 8u * j < nrows) ? *p : 0.0f;
                    p += step;
                }
            }
        };
        auto stage = [&]() {
            if (vec_in) {
#pragma unroll
                for (int j = 0; j < GZ_GC / 4; ++j) {
                    const unsigned q = tid + 256u * j;
                    if (q < tile_q) {
                        float *d = &xs[(q >> 3) * GZ_XS + 4 * (q & 7)];
                        d[0] = xv[4 * j];
                        d[1] = xv[4 * j + 1];
                        d[2] = xv[4 * j + 2];
                        d[3] = xv[4 * j + 3];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < GZ_GC; ++j) {
                    const unsigned q = tid + 256u * j;
                    if (q < tile_q) xs[(q >> 5) * GZ_XS + (q & 31)] = xv[j];
                }
            }
        };

        const bool live = lane_ok && row0 + r < batch;
        const float *row = &xs[(live ? r : 0) * GZ_XS];
        float s1 = 0.0f, s2 = 0.0f;  // s_prev, s_prev2 (goertzel.rs:27-28)
        load(0);
        for (int i0 = 0; i0 < n; i0 += GZ_GC) {
            stage();
            __syncthreads();
            if (i0 + GZ_GC < n) load(i0 + GZ_GC);  // in flight while this chunk is computed
            const int cnt = n - i0 < GZ_GC ? n - i0 : GZ_GC;
            if (live) {
                if (cnt == GZ_GC) {
#pragma unroll
                    for (int ii = 0; ii < GZ_GC; ++ii) {
                        const float s = (row[ii] + c * s1) - s2;  // goertzel.rs:30
                        s2 = s1;
                        s1 = s;
                    }
                } else {
                    for (int ii = 0; ii < cnt; ++ii) {
                        const float s = (row[ii] + c * s1) - s2;
                        s2 = s1;
                        s1 = s;
                    }
                }
            }
            __syncthreads();
        }
        if (live) out[(row0 + r) * (size_t)nfreq + f] = spectral_root_cr((s2 * s2 + s1 * s1) - (c * s1) * s2);  // goertzel.rs:34-35
    }
}

}  // namespace host
}  // namespace kofft
