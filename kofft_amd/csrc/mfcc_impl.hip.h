// mfcc_impl.hip.h -- cepstrum::mel_filterbank and cepstrum::mfcc (cepstrum.rs:36-85) on device pointers, f32 only like the reference,
// with the filter edges as an input (include/kofft_hip.h: what is pinned and what is not).
//
// The host turns the edges into a plan (kofft_tables::mel_plan_build): the segments [bins[s], bins[s + 1]) clamped to the row, the
// live flag of every filter and, per k, the two weights the reference computes there -- the rise weight of filter s and the fall
// weight of filter s - 1, for the segment s that holds k.  The plan is the same for every row, so a LANE OWNS A ROW and nothing in
// the walk over k diverges: one ascending sweep carries two accumulators, `rise` (filter s) and `fall` (filter s - 1); per element
// it does fall += w_fall * x, rise += w_rise * x (one multiply, one add each, never fused); at the end of segment s filter s - 1 is
// complete (its rise terms in segment s - 1, then its fall terms in segment s: the reference's order) and rise becomes the next
// segment's fall.  A dead filter (an empty rise or fall) accumulates like any other and is replaced by +0 when it is emitted; no sum
// is ever split.
//
// mel_kernel<VEC, FUSED>: one wavefront per workgroup, 64 rows.  The rows lie n_fft floats apart, so the magnitudes come in through
// LDS: a tile of 64 rows x MEL_KC values of k is loaded coalesced (VEC: 16 bytes per lane, a 16-byte aligned input and n_fft % 4 == 0;
// else 4 bytes per lane), the next tile's loads are in flight while this one is summed, and a lane reads its row back with the row
// stride MEL_KC + 1 (ds_read_b32 banks by 32: the 32 lanes of a half hit 32 banks).  Results leave through a tile of 64 rows x MEL_OC
// values, flushed with 128-byte runs per row.
//  * FUSED = false writes the energies (kofft_hip_dev_mel_filterbank_f32, and step 1 of the composed MFCC);
//  * FUSED = true keeps going in the same lane: logf(e + 1e-12f) of every filter into the lane's own LDS column, then the truncated
//    DCT-II from the cached direct table, whose rows are the same for every lane (scalar loads), eight outputs per pass over the
//    column.  Energies never reach memory.  LDS: one tile of 64 x 33 floats (input, then output) + 256 bytes per filter: 40.25 KiB
//    at the 128 filters it is built for (three workgroups per CU), 18.25 KiB at 40.
// The composed MFCC (num_mel > kMfccFusedMaxMel; by the measured default also num_mel > kMfccFusedDefaultMel or num_coeffs >
// kMfccFusedDefaultCoeffs; every call after kofft_hip_set_mfcc_fused(ctx, 0)): mel_kernel<., false> into the context's
// scratch, mel_log_kernel in place, direct_dev(DCT-II) on rows of num_mel, mel_cols_kernel.  The same operations per value.
#pragma once

#include "direct_impl.hip.h"
#include "libm_logf.hip.h"

namespace kofft {
namespace host {

constexpr int MEL_ROWS = 64;          // rows per workgroup: one per lane
constexpr int MEL_KC = 32;            // values of k per tile
constexpr int MEL_OC = 32;            // results per row in the output tile
constexpr int MEL_TS = MEL_KC + 1;    // row strides of the two tiles
constexpr int MEL_OS = MEL_OC + 1;
constexpr int MEL_JB = 8;             // DCT outputs per pass over the log-mel column

inline size_t mel_lds_bytes(bool fused, size_t num_mel)
{
    // (fused: the results leave after the sweep, through the input tile's space)
    return fused ? (size_t)MEL_ROWS * MEL_TS * sizeof(float) + num_mel * MEL_ROWS * sizeof(float)
                 : (size_t)(MEL_ROWS * MEL_TS + MEL_ROWS * MEL_OS) * sizeof(float);
}

typedef float mel_f4 __attribute__((ext_vector_type(4)));

// plan: [seg: 2 (num_mel + 1) ints | live: num_mel ints | w: 2 n_fft floats] (tables.h); dct: the DCT-II direct table of num_mel,
// row stride ldc (FUSED only); out: rows x num_mel energies, or rows x nc coefficients (FUSED)
template <bool VEC, bool FUSED>
__global__ __launch_bounds__(MEL_ROWS) void mel_kernel(const float *__restrict__ x, float *__restrict__ out, const int *__restrict__ plan,
                                                       const float *__restrict__ dct, const int n_fft, const int num_mel, const int nc,
                                                       const int ldc, const size_t rows)
{
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    float *tile = mel_lds;
    static_assert(MEL_OS <= MEL_TS, "the fused kernel's output tile lies in the input tile");
    float *ot = FUSED ? tile : tile + MEL_ROWS * MEL_TS;
    float *lm = tile + MEL_ROWS * MEL_TS;  // (FUSED) lm[m * 64 + lane]
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * MEL_ROWS;
    const int nrows = rows - row0 < (size_t)MEL_ROWS ? (int)(rows - row0) : MEL_ROWS;
    const int *seg = plan, *live = plan + 2 * (num_mel + 1);
    const float *w = reinterpret_cast<const float *>(plan + 2 * (num_mel + 1) + num_mel);
    const float *xb = x + row0 * (size_t)n_fft;

    // ---- the way out: results [o0, o0 + ocount) of every row wait in `ot` ----
    const int outlen = FUSED ? nc : num_mel;
    float *ob = out + row0 * (size_t)outlen;
    int o0 = 0, ocount = 0;
    auto flush = [&]() {
        __syncthreads();
        const int c = lane & (MEL_OC - 1), rs = lane >> 5;
#pragma unroll 4
        for (int r2 = 0; r2 < MEL_ROWS / 2; ++r2) {
            const int r = 2 * r2 + rs;
            if (r < nrows && c < ocount) ob[(size_t)r * outlen + o0 + c] = ot[r * MEL_OS + c];
        }
        __syncthreads();
        o0 += ocount;
        ocount = 0;
    };
    auto put = [&](const float v) {
        ot[lane * MEL_OS + ocount] = v;
        if (++ocount == MEL_OC) flush();
    };

    // ---- the way in: the tile [t0, t0 + MEL_KC) of the 64 rows, through registers ----
    constexpr int NLD = VEC ? MEL_ROWS * MEL_KC / 4 / 64 : MEL_ROWS * MEL_KC / 64;
    mel_f4 v4[VEC ? NLD : 1];
    float v1[VEC ? 1 : NLD];
    auto load = [&](const int t0) {
        if constexpr (VEC) {
            const int kk = 4 * (lane & 7), rs = lane >> 3;
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int r = 8 * j + rs;
                const bool ok = r < nrows && t0 + kk < n_fft;  // (n_fft % 4 == 0: the four values are in the row together)
                v4[j] = ok ? *reinterpret_cast<const mel_f4 *>(xb + (size_t)r * n_fft + t0 + kk) : mel_f4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        } else {
            const int kk = lane & (MEL_KC - 1), rs = lane >> 5;
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int r = 2 * j + rs;
                v1[j] = (r < nrows && t0 + kk < n_fft) ? xb[(size_t)r * n_fft + t0 + kk] : 0.0f;
            }
        }
    };
    auto stage = [&]() {
        if constexpr (VEC) {
            const int kk = 4 * (lane & 7), rs = lane >> 3;
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                float *t = tile + (8 * j + rs) * MEL_TS + kk;
                t[0] = v4[j].x;
                t[1] = v4[j].y;
                t[2] = v4[j].z;
                t[3] = v4[j].w;
            }
        } else {
            const int kk = lane & (MEL_KC - 1), rs = lane >> 5;
#pragma unroll
            for (int j = 0; j < NLD; ++j) tile[(2 * j + rs) * MEL_TS + kk] = v1[j];
        }
    };

    // ---- the sweep ----
    float rise = 0.0f, fall = 0.0f;
    int s = 0;  // the segment the sweep is in
    auto end_segment = [&]() {
        if (s >= 1) {
            const float e = live[s - 1] ? fall : 0.0f;
            if constexpr (FUSED) lm[(s - 1) * MEL_ROWS + lane] = libm_logf(e + 1e-12f);  // cepstrum.rs:82
            else put(e);
        }
        fall = rise;
        rise = 0.0f;
        ++s;
    };
    const int kbeg = seg[0], kend = seg[2 * num_mel + 1];
    const int tfirst = kbeg / MEL_KC * MEL_KC;
    if (kbeg < kend) load(tfirst);
    for (int t0 = tfirst; t0 < kend; t0 += MEL_KC) {
        __syncthreads();
        stage();
        __syncthreads();
        if (t0 + MEL_KC < kend) load(t0 + MEL_KC);  // in flight while this tile is summed
        int k = t0 > kbeg ? t0 : kbeg;
        const int te = t0 + MEL_KC < kend ? t0 + MEL_KC : kend;
        const float *mine = tile + lane * MEL_TS;
        while (k < te) {
            while (k >= seg[2 * s + 1]) end_segment();
            const int hi = seg[2 * s + 1];
            const int e = te < hi ? te : hi;
            for (; k < e; ++k) {
                const float xv = mine[k - t0];
                const float tr = w[2 * k] * xv;      // cepstrum.rs:59
                const float tf = w[2 * k + 1] * xv;  // cepstrum.rs:64
                rise = rise + tr;
                fall = fall + tf;
            }
        }
    }
    while (s <= num_mel) end_segment();

    if constexpr (FUSED) {
        __syncthreads();  // the input tile becomes the output tile
        // dct::dct2 of the lane's column, outputs j < nc (dct.rs:134-146).  The table's rows are padded with zeros to ldc, a multiple
        // of 128: the eight outputs of a pass are in the row together.
        for (int j0 = 0; j0 < nc; j0 += MEL_JB) {
            float acc[MEL_JB];
#pragma unroll
            for (int t = 0; t < MEL_JB; ++t) acc[t] = 0.0f;
            for (int i = 0; i < num_mel; ++i) {
                const float l = lm[i * MEL_ROWS + lane];
                const float *c = dct + (size_t)i * ldc + j0;
#pragma unroll
                for (int t = 0; t < MEL_JB; ++t) {
                    const float term = l * c[t];
                    acc[t] = acc[t] + term;
                }
            }
#pragma unroll
            for (int t = 0; t < MEL_JB; ++t)
                if (j0 + t < nc) put(acc[t]);
        }
    }
    if (ocount) flush();
}

// ---- composed route: the pointwise step and the column copy, flat grid-stride grids -----------------------------------------------
__global__ __launch_bounds__(256) void mel_log_kernel(float *__restrict__ v, const size_t total)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) v[i] = libm_logf(v[i] + 1e-12f);
}

// out[r][j] = src[r][j], j < nc, rows of num_mel in, rows of nc out (cepstrum.rs:84).  The lanes as in direct_simple_kernel: rpb =
// 256 / nc rows per workgroup (nc < 256: one 32-bit division) or 256 columns of one row; blockIdx.y strides over the row groups.
__global__ __launch_bounds__(256) void mel_cols_kernel(const float *__restrict__ src, float *__restrict__ out, const unsigned num_mel,
                                                       const unsigned nc, const size_t rows, const unsigned rpb)
{
    const unsigned tid = threadIdx.x;
    unsigned r = 0, j = blockIdx.x * 256u + tid;
    if (rpb > 1) {
        r = tid / nc;
        j = tid - r * nc;
        if (r >= rpb) return;
    }
    if (j >= nc) return;
    for (size_t b = (size_t)blockIdx.y * rpb + r; b < rows; b += (size_t)gridDim.y * rpb) out[b * nc + j] = src[b * num_mel + j];
}

}  // namespace host
}  // namespace kofft
