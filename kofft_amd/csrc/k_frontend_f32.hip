// k_frontend_f32.hip -- rows of audio to mel energies or MFCCs in one call (frontend_impl.hip.h): every kernel
// instance of the family, the argument checks, the two routes and the extern "C" entry points.
#include "frontend_impl.hip.h"
#include "host_stage.hip.h"

#include "direct_impl.hip.h"

namespace kofft {
namespace host {

// the magnitudes kernels without a maximum run their parents' configurations
template <> struct PersistCfg<10, StftMagRowsNoMaxIO> : PersistCfg<10, StftMagIO> {};
template <> struct PersistCfg<11, StftMagRowsNoMaxIO> : PersistCfg<11, StftMagIO> {};
template <> struct PersistCfg<12, StftMagRowsNoMaxIO> : PersistCfg<12, StftMagIO> {};

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched: the STFT rows' first, then the mel ones.
static int frontend_check(bool mfcc, bool dev, const void *signal, const void *window, const void *out, size_t rows, size_t len, size_t row_stride,
                   size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs, const kofft_hip_ctx *ctx)
{
    const int crc = stft_rows_check(true, true, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (mfcc && num_coeffs > num_mel) return KOFFT_ERR_INVALID_VALUE;  // cepstrum.rs:79
    if (!bins) return KOFFT_ERR_NULL;
    for (size_t i = 0; i < num_mel + 1 && i + 1 != 0; ++i)
        if (bins[i + 1] < bins[i]) return KOFFT_ERR_INVALID_VALUE;
    if (win_len / 2 > kMelMaxFft || num_mel > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !out || (!signal && len)) return KOFFT_ERR_NULL;
    if (dev) {
        const size_t out_row = mfcc ? num_coeffs : num_mel;
        const size_t out_bytes = rows * frames * out_row * sizeof(float);
        if (overlaps(out, out_bytes, signal, rows_span(rows, len, row_stride) * sizeof(float))) return KOFFT_ERR_INVALID_VALUE;
        if (overlaps(out, out_bytes, window, win_len * sizeof(float))) return KOFFT_ERR_INVALID_VALUE;
    }
    return KOFFT_OK;
}

// ---- the fused route ---------------------------------------------------------------------------------------------------------------
constexpr size_t kFrontendFusedMinWin = 64, kFrontendFusedMaxWin = 2048;  // fft_wg_kernel's window lengths with room for the log-mel rows

static bool frontend_fused_fits(size_t win_len, size_t num_mel)
{
    return is_pow2(win_len) && win_len >= kFrontendFusedMinWin && win_len <= kFrontendFusedMaxWin && num_mel <= kMfccFusedMaxMel;
}

// Mode 1 takes the fused kernel only where it beat the two-call chain by more than the spread of the runs at every batch measured
// AND is not slower than the composed route.  Measured on an MI355X: it beats the chain at win_len 64 .. 512 with
// 40 x 13 (10-14 % at 1024 rows), loses to it at config 4's stream (0.315 against 0.220 ms) and loses to the composed route at every
// shape by 21-51 % (the generic workgroup kernel against the persistent magnitudes kernels, and an epilogue that leaves most lanes
// idle).  So no shape takes it by default; it stays behind mode 2.
static bool frontend_use_fused(const kofft_hip_ctx *ctx, size_t win_len, size_t num_mel, size_t num_coeffs)
{
    (void)num_coeffs;
    if (ctx->frontend_fused == 0 || !frontend_fused_fits(win_len, num_mel)) return false;
    return ctx->frontend_fused == 2;
}

template <int L, bool MFCC>
static int launch_frontend(kofft_hip_ctx *ctx, const FrontendIO<MFCC> &io, const cpx<float> *tw, size_t batch)
{
    constexpr int RL = rl_for(L), TPT = (1 << L) >> RL, BLOCK = TPT > 256 ? TPT : 256, XPB = BLOCK / TPT;
    constexpr size_t slots = lds_wg_bytes<float, false, false, XPB>(1 << L);
    static_assert(slots + XPB * kMfccFusedMaxMel * sizeof(float) <= 64 * 1024, "LDS without an attribute");
    const size_t lds = slots + (MFCC ? (size_t)XPB * io.num_mel * sizeof(float) : 0);
    const size_t blocks = (batch + XPB - 1) / XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((fft_wg_kernel<float, L, RL, BLOCK, EPI_MEL, FrontendIO<MFCC>>), dim3((unsigned)blocks), dim3(BLOCK), lds, ctx->stream, io,
                       tw, batch);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

template <bool MFCC>
static int frontend_fused(kofft_hip_ctx *ctx, const FramedSrc &s, const uint64_t *bins, size_t num_mel, size_t nc, float *d_out)
{
    const size_t win_len = s.win_len;
    const int *plan = nullptr;
    int rc = get_mel_plan(ctx, bins, win_len / 2, num_mel, &plan);
    if (rc) return rc;
    const float *table = nullptr;
    if (MFCC) {
        rc = get_direct_table(ctx, 0, 2, num_mel, &table);  // the cache entry of kofft_hip_dct_direct_f32(ctx, 2, ..) at n = num_mel
        if (rc) return rc;
    }
    const cpx<float> *tw = nullptr;
    rc = twiddle_table<float>(ctx, win_len, &tw);
    if (rc) return rc;
    FrontendIO<MFCC> io{};
    fill_rows_io(io, s);
    io.plan = plan;
    io.dct = table;
    io.res = d_out;
    io.num_mel = (int)num_mel;
    io.nc = (int)nc;
    io.ldc = (int)direct_ldc(num_mel);
    const size_t batch = s.rows * s.frames;
    // (never outside 6 .. 11: frontend_fused_fits)
    return dispatch_log2<6, 11>(ilog2(win_len), [&](auto l) { return launch_frontend<decltype(l)::value, MFCC>(ctx, io, tw, batch); });
}

// ---- the composed route ------------------------------------------------------------------------------------------------------------
// magnitudes of frames [f0, f0 + nf) of each of nrows rows (f0 != 0: one row), dense at d_mags, no maximum
int mags_piece(kofft_hip_ctx *ctx, const float *d_signal, size_t nrows, size_t len, size_t row_stride, const float *d_win, size_t win_len,
                      size_t hop, size_t f0, size_t nf, float *d_mags)
{
    StftMagRowsNoMaxIO io{};
    fill_rows_io(io, d_signal, nrows, len, row_stride, d_win, win_len, hop, nf);
    io.start0 = (f0 && hop > len / f0) ? len : f0 * hop;  // (a start at or past len: silence, as every frame after it)
    io.mags = d_mags;
    io.max_bits = nullptr;
    return dispatch<float, EPI_STORE>(ctx, io, win_len, nrows * nf);
}

// Whole frames of the flat index t = row * frames + frame, scratch_chunk_bytes of scratch at a time: [magnitudes | (window lengths the
// magnitudes kernels do not cover) the composed frames].  A chunk may begin and end inside a row (framed_produce cuts it).
static int frontend_composed(kofft_hip_ctx *ctx, bool mfcc, const FramedSrc &s, const uint64_t *bins, size_t num_mel, size_t nc, float *d_out)
{
    const size_t win_len = s.win_len, half = win_len / 2, total = s.rows * s.frames, out_row = mfcc ? nc : num_mel;
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, half * sizeof(float) + (s.kernels ? 0 : win_len * sizeof(cpx<float>)), total);
    const size_t mags_bytes = (chunk * half * sizeof(float) + 15) & ~size_t(15);
    const int erc = ensure(ctx, ctx->rows_tmp, mags_bytes + (s.kernels ? 0 : chunk * win_len * sizeof(cpx<float>)) + 16);
    if (erc) return erc;
    float *mags = static_cast<float *>(ctx->rows_tmp.p);
    cpx<float> *spec = reinterpret_cast<cpx<float> *>(static_cast<char *>(ctx->rows_tmp.p) + mags_bytes);
    return for_chunks(total, chunk, [&](size_t t0, size_t nt) {
        const int rc = half ? framed_produce(ctx, s, FRAMES_MAGS, t0, nt, mags, spec) : KOFFT_OK;  // (a one-sample window has no bins)
        if (rc) return rc;
        return mfcc ? mfcc_dev(ctx, mags, d_out + t0 * out_row, half, nt, bins, num_mel, nc)
                    : mel_filterbank_dev(ctx, mags, d_out + t0 * out_row, half, nt, bins, num_mel);
    });
}

static int frontend_dev(kofft_hip_ctx *ctx, bool mfcc, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                 size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs, float *d_out)
{
    const int crc = frontend_check(mfcc, true, d_signal, d_window, d_out, rows, len, row_stride, win_len, hop, frames, bins, num_mel, num_coeffs, ctx);
    if (crc || rows == 0 || frames == 0 || num_mel == 0 || (mfcc && num_coeffs == 0)) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    FramedSrc s;
    const int rc = framed_src(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, &s);
    if (rc) return rc;
    if (frontend_use_fused(ctx, win_len, num_mel, num_coeffs))
        return mfcc ? frontend_fused<true>(ctx, s, bins, num_mel, num_coeffs, d_out) : frontend_fused<false>(ctx, s, bins, num_mel, 0, d_out);
    return frontend_composed(ctx, mfcc, s, bins, num_mel, num_coeffs, d_out);
}

// The signal goes up, the energies or coefficients come down (whole rows per chunk of the pipeline); the magnitudes stay on the device.
static int frontend_host(kofft_hip_ctx *ctx, bool mfcc, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                         size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs, float *out)
{
    const int crc = frontend_check(mfcc, false, signal, window, out, rows, len, row_stride, win_len, hop, frames, bins, num_mel, num_coeffs, ctx);
    if (crc || rows == 0 || frames == 0 || num_mel == 0 || (mfcc && num_coeffs == 0)) return crc;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, len, frames * (mfcc ? num_coeffs : num_mel), window, window ? win_len : 0, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return frontend_dev(ctx, mfcc, d_in, nb, len, len, d_win, win_len, hop, frames, bins, num_mel, num_coeffs, d_out);
                            });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_stft_mel_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                           size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, float *energies)
{
    return frontend_host(ctx, false, signal, rows, len, row_stride, window, win_len, hop, frames, bins, num_mel, 0, energies);
}

int kofft_hip_dev_stft_mel_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                               size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, float *d_energies)
{
    return frontend_dev(ctx, false, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins, num_mel, 0, d_energies);
}

int kofft_hip_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                            size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs, float *coeffs)
{
    return frontend_host(ctx, true, signal, rows, len, row_stride, window, win_len, hop, frames, bins, num_mel, num_coeffs, coeffs);
}

int kofft_hip_dev_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                                size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs,
                                float *d_coeffs)
{
    return frontend_dev(ctx, true, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins, num_mel, num_coeffs, d_coeffs);
}

int kofft_hip_set_frontend_fused(kofft_hip_ctx *ctx, int mode) { return set_route(ctx, &kofft_hip_ctx::frontend_fused, mode, 0, 2); }

}  // extern "C"
