// frontend_impl.hip.h -- rows of audio to mel energies or MFCCs in one call: stft_magnitudes (visual/spectrogram.rs:52-76)
// -> cepstrum::mel_filterbank -> logf -> dct::dct2 (cepstrum.rs:36-85), f32 only like the reference.  Two routes, the same bytes:
//
//  * FUSED: fft_wg_kernel<float, L, RL, BLOCK, EPI_MEL, FrontendIO<MFCC>>.  The input side is StftRowsOf<StftIO> unchanged (frame
//    bounds per row, the descriptor loads, the window); after the last stage every thread holds R outputs of its frame and the
//    policy's epilogue finishes the workgroup's XPB frames from LDS:
//      1. the magnitude sqrtf(re*re + im*im) of every kept bin o < n/2 into the frame's own exchange slot, natural order, one f32 each
//         (the discarded half is never rooted or stored);
//      2. a lane per (frame, filter) walks its filter over the frame's magnitudes (frontend_walk.h: rise terms, then fall terms, the
//         reference's order); energies: stored from here, the workgroup's XPB * num_mel floats are one contiguous run and lane e
//         stores element e of it; MFCC: libm_logf(e + 1e-12f) into the log-mel rows behind the exchange slots;
//      3. (MFCC) a lane per (frame, j) sums lm[i] * C[i][j] ascending i from +0 over the cached direct DCT-II table (rows padded to
//         128 floats, as mel_kernel relies on) and stores element e of the workgroup's XPB * num_coeffs floats.
//    Frames of different rows are adjacent in the dense output, so a run is contiguous across a row seam too.  The magnitudes never
//    reach memory.  LDS: the exchange slots XPB * lds_elems(n) * 8 bytes + (MFCC) XPB * num_mel * 4.
//  * COMPOSED: the existing magnitudes kernels with an accumulator that compiles away (StftMagRowsNoMaxIO: no maximum is computed),
//    whole frames at a time into the context's scratch, then the mel / MFCC device path on that scratch.
#pragma once

#include "frontend_walk.h"
#include "host_common.hip.h"
#include "libm_logf.hip.h"

namespace kofft {

// stft_magnitudes over rows WITHOUT the maximum: StftMagRowsIO's stores, an empty accumulator.  max_bits stays null and is never read.
struct StftMagRowsNoMaxIO : StftRowsOf<StftMagIO> {
    static constexpr bool kRowAcc = true;
    struct Acc {};
    __device__ __forceinline__ Acc acc_init() const { return Acc{}; }
    __device__ __forceinline__ void acc_finish(Acc) const {}
    __device__ __forceinline__ void acc_row(size_t, float) const {}
    __device__ __forceinline__ void store_acc(size_t xf, int o, cpx<float> v, Acc &) const
    {
        if (o < n / 2) st_stream(mags + xf * (size_t)(n / 2) + o, sqrtf(sumsq(v)));
    }
    __device__ __forceinline__ void store_d_acc(rsrc_t d, int lane_bytes, int ou, cpx<float> v, int row_off, Acc &) const
    {
        if (ou + (lane_bytes >> 3) < n / 2) buf_store_f32(sqrtf(sumsq(v)), d, row_off + (lane_bytes >> 1), ou * 4);
    }
};

// The fused kernel's policy: StftRowsIO's input side, the epilogue below instead of stores.
template <bool MFCC>
struct FrontendIO : StftRowsOf<StftIO> {
    const int *__restrict__ plan;   // [seg | live | w] of (bins, n/2, num_mel) (kofft_tables::mel_plan_build)
    const float *__restrict__ dct;  // (MFCC) the direct DCT-II table of num_mel, row stride ldc
    float *__restrict__ res;        // batch x num_mel energies, or batch x nc coefficients
    int num_mel, nc, ldc;

    template <int L, int RL, int BLOCK>
    __device__ __forceinline__ void mel_epilogue(const cpx<float> *v, char *smem, const size_t blk, const size_t batch, const int tau,
                                                 const int slot) const
    {
        constexpr int N = 1 << L, R = 1 << RL, TPT = N / R, XPB = BLOCK / TPT, NP = (L + RL - 1) / RL, H = N / 2;
        constexpr int SLOTF = 2 * lds_elems(N);  // floats of one exchange slot
        static_assert(H <= SLOTF, "a frame's magnitudes fit its slot");
        using GL = WgGeom<L, RL, NP - 1>;
        float *slots = reinterpret_cast<float *>(smem);
        float *lm = slots + XPB * SLOTF;  // (MFCC) lm[frame * num_mel + filter]
        const int tid = threadIdx.x;
        const size_t xf0 = blk * XPB;
        const int cnt = batch - xf0 < (size_t)XPB ? (int)(batch - xf0) : XPB;  // frames of this workgroup that exist (>= 1)

        // 1. magnitudes of the kept half (spectrogram.rs:63-66); a slot past the batch holds the transform of zeros and is never emitted
        float *mine = slots + slot * SLOTF;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int o = GL::out_index(tau, u);
            if (o < H) mine[o] = sqrtf(v[u].re * v[u].re + v[u].im * v[u].im);
        }
        __syncthreads();

        // 2. the filterbank (cepstrum.rs:52-70): element e = frame * num_mel + filter
        const float *w = reinterpret_cast<const float *>(plan + 2 * (num_mel + 1) + num_mel);
        float *run = res + xf0 * (size_t)(MFCC ? nc : num_mel);
        for (int e = tid; e < cnt * num_mel; e += BLOCK) {
            const int f = e / num_mel, m = e - f * num_mel;
            const float en = frontend_filter_walk(plan, w, slots + f * SLOTF, num_mel, m);
            if constexpr (MFCC) lm[e] = libm_logf(en + 1e-12f);  // cepstrum.rs:82
            else run[e] = en;
        }
        if constexpr (MFCC) {
            __syncthreads();
            // 3. dct::dct2 of every log-mel row, outputs j < nc (dct.rs:134-146): element e = frame * nc + j
            for (int e = tid; e < cnt * nc; e += BLOCK) {
                const int f = e / nc, j = e - f * nc;
                const float *l = lm + f * num_mel;
                const float *c = dct + j;
                float acc = 0.0f;
                for (int i = 0; i < num_mel; ++i) {
                    const float term = l[i] * c[(size_t)i * ldc];
                    acc = acc + term;
                }
                run[e] = acc;
            }
        }
    }
};

}  // namespace kofft
