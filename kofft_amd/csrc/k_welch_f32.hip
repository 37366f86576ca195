// k_welch_f32.hip -- Welch power spectra and cross spectra of rows (welch_impl.hip.h): every kernel instance of the
// family, the argument checks and the two routes.
#include "welch_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched: the STFT rows' without the frame count,
// then the flags, the pointers, the overlaps.
static int welch_check(bool csd, const void *x, const void *y, const void *window, const void *out, size_t rows, size_t len, size_t row_stride,
                size_t win_len, size_t hop, size_t frames, int flags, const kofft_hip_ctx *ctx)
{
    const int crc = stft_rows_check(false, false, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (flags & ~KOFFT_HIP_PSD_DOUBLE) return KOFFT_ERR_INVALID_VALUE;
    if (!ctx || !out || (len && (!x || (csd && !y)))) return KOFFT_ERR_NULL;
    const size_t out_bytes = rows * (win_len / 2 + 1) * (csd ? 2 : 1) * sizeof(float), in_bytes = rows_span(rows, len, row_stride) * sizeof(float);
    if (overlaps(out, out_bytes, x, in_bytes)) return KOFFT_ERR_INVALID_VALUE;
    if (csd && overlaps(out, out_bytes, y, in_bytes)) return KOFFT_ERR_INVALID_VALUE;
    if (overlaps(out, out_bytes, window, win_len * sizeof(float))) return KOFFT_ERR_INVALID_VALUE;
    return KOFFT_OK;
}

// ---- the fused route ---------------------------------------------------------------------------------------------------------------
constexpr size_t kWelchFusedMinWin = 64, kWelchFusedMaxWin = 4096;

static bool welch_fused_fits(size_t win_len)
{
    return is_pow2(win_len) && win_len >= kWelchFusedMinWin && win_len <= kWelchFusedMaxWin;
}

// Mode 1: the measured choice per window length: the fused kernel wherever it was not slower than the composed route
// beyond the spread of the runs at every shape tried.  Measured on an MI355X: it is 1.05 to 3.2 times faster at win_len 64 .. 1024 and
// 4096 (power and cross spectrum, every shape), and loses at 2048 -- the power spectrum at all four shapes tried (0.175 against 0.157 ms
// at 64 x 480 000, 0.150 against 0.086 at 16 x 1 000 000: two waves per workgroup and few groups against the persistent STFT kernel's
// frame-level parallelism), the cross spectrum at one of them (0.192 against 0.158).  So 2048 stays behind mode 2.
static bool welch_use_fused(const kofft_hip_ctx *ctx, size_t win_len)
{
    if (ctx->welch_fused == 0 || !welch_fused_fits(win_len)) return false;
    return ctx->welch_fused == 2 || win_len != 2048;
}

struct WelchCall {
    FramedSrc src;   // of x; src.frames: the frames that can hold a sample, at least 1
    const float *y;  // the cross spectrum only
    bool csd;
    size_t ngroups;
    float scale;
    int twice;
    float *out;
};

static int launch_total(kofft_hip_ctx *ctx, const WelchCall &c, const float *part, size_t g_first, size_t g_count)
{
    const size_t win_len = c.src.win_len, K = win_len / 2 + 1, vals = K * (c.csd ? 2 : 1);
    const size_t nrows = (g_first + g_count - 1) / c.ngroups - g_first / c.ngroups + 1;
    const size_t blocks = (nrows * vals + 255) / 256;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(welch_total_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, part, c.out, vals, c.csd ? 2 : 1, c.ngroups, g_first,
                       g_count, c.scale, c.twice, (win_len & 1) ? K : K - 1, nrows * vals);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

template <int L, bool CSD>
static int launch_fused(kofft_hip_ctx *ctx, const WelchCall &c, const cpx<float> *tw, size_t g_first, size_t g_count, float *dst, bool final)
{
    constexpr int RL = rl_for(L), TPT = (1 << L) >> RL, BLOCK = TPT > 64 ? TPT : 64, XPB = BLOCK / TPT;
    constexpr size_t lds = lds_wg_bytes<float, false, false, XPB>(1 << L);
    static_assert(lds <= 64 * 1024, "LDS without an attribute");
    const size_t blocks = (g_count + XPB - 1) / XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    StftIO io{};
    io.signal = c.src.signal;
    io.window = c.src.win;
    io.out = nullptr;
    io.len = c.src.len;
    io.hop = c.src.hop;
    io.start0 = 0;
    io.n = 1 << L;
    hipLaunchKernelGGL((welch_fused_kernel<L, RL, BLOCK, CSD>), dim3((unsigned)blocks), dim3(BLOCK), lds, ctx->stream, io, c.y, tw, c.src.row_stride,
                       c.src.frames, c.ngroups, g_first, g_count, dst, c.scale, c.twice, final ? 1 : 0);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

template <bool CSD>
static int launch_fused_l(kofft_hip_ctx *ctx, const WelchCall &c, const cpx<float> *tw, size_t g_first, size_t g_count, float *dst, bool final)
{
    // (never outside 6 .. 12: welch_fused_fits)
    return dispatch_log2<6, 12>(ilog2(c.src.win_len),
                                [&](auto l) { return launch_fused<decltype(l)::value, CSD>(ctx, c, tw, g_first, g_count, dst, final); });
}

// Rows of one group: one launch, scaled from the kernel.  Otherwise the partials of at most scratch_chunk_bytes of groups at a time,
// then their rows' totals.
static int welch_fused(kofft_hip_ctx *ctx, const WelchCall &c)
{
    const cpx<float> *tw = nullptr;
    int rc = twiddle_table<float>(ctx, c.src.win_len, &tw);
    if (rc) return rc;
    const size_t vals = (c.src.win_len / 2 + 1) * (c.csd ? 2 : 1), total = c.src.rows * c.ngroups;
    const auto launch = c.csd ? launch_fused_l<true> : launch_fused_l<false>;
    if (c.ngroups == 1)
        return for_chunks(total, size_t(1) << 30, [&](size_t g0, size_t ng) { return launch(ctx, c, tw, g0, ng, c.out, true); });
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, vals * sizeof(float), total);
    rc = ensure(ctx, ctx->rows_tmp, chunk * vals * sizeof(float));
    if (rc) return rc;
    float *part = static_cast<float *>(ctx->rows_tmp.p);
    return for_chunks(total, chunk, [&](size_t g0, size_t ng) {
        const int lrc = launch(ctx, c, tw, g0, ng, part, false);
        return lrc ? lrc : launch_total(ctx, c, part, g0, ng);
    });
}

// ---- the composed route ------------------------------------------------------------------------------------------------------------
// Chunks of whole groups (welch_cut.h) through the scratch: [frames of x | frames of y | partials], at most scratch_chunk_bytes (one
// group where a group alone is larger).  The frames are framed_produce's: the one-sided frames where the STFT kernels cover the window
// length, otherwise the full composed frames, read in place.
static int welch_composed(kofft_hip_ctx *ctx, const WelchCall &c)
{
    const FramedSrc &sx = c.src;
    FramedSrc sy = c.src;
    sy.signal = c.y;
    const bool kernels = sx.kernels, csd = c.csd;
    const FramedForm form = kernels ? FRAMES_HALF : FRAMES_FULL;
    const size_t K = sx.win_len / 2 + 1, vals = K * (csd ? 2 : 1), fstride = kernels ? K : sx.win_len, total = sx.rows * sx.frames;
    const size_t per_frame = fstride * sizeof(cpx<float>) * (csd ? 2 : 1) + (vals * sizeof(float) + kWelchGroup - 1) / kWelchGroup;
    size_t cap = scratch_chunk_rows(ctx->scratch_chunk_bytes, per_frame, total);
    if (cap < kWelchGroup) cap = kWelchGroup < total ? kWelchGroup : total;
    size_t max_groups = cap / kWelchGroup + cap / sx.frames + 2;  // whole groups, one short group per row end, the two ends
    if (max_groups > sx.rows * c.ngroups) max_groups = sx.rows * c.ngroups;
    const size_t spec_bytes = (cap * fstride * sizeof(cpx<float>) + 15) & ~size_t(15);
    int rc = ensure(ctx, ctx->rows_tmp, spec_bytes * (csd ? 2 : 1) + max_groups * vals * sizeof(float));
    if (rc) return rc;
    char *base = static_cast<char *>(ctx->rows_tmp.p);
    cpx<float> *spec_x = reinterpret_cast<cpx<float> *>(base), *spec_y = csd ? reinterpret_cast<cpx<float> *>(base + spec_bytes) : nullptr;
    float *part = reinterpret_cast<float *>(base + spec_bytes * (csd ? 2 : 1));
    for (size_t t0 = 0; t0 < total;) {
        const size_t end = welch_chunk_end(t0, cap, sx.frames, total), nt = end - t0;
        const size_t g0 = welch_group_at(t0, sx.frames), ng = (end == total ? sx.rows * c.ngroups : welch_group_at(end, sx.frames)) - g0;
        if (ng > max_groups) return KOFFT_ERR_UNSUPPORTED;  // (never: the bound above)
        rc = framed_produce(ctx, sx, form, t0, nt, spec_x, nullptr);
        if (rc) return rc;
        if (csd) {
            rc = framed_produce(ctx, sy, form, t0, nt, spec_y, nullptr);
            if (rc) return rc;
        }
        const size_t blocks = (ng * K + 255) / 256;
        if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
        if (csd)
            hipLaunchKernelGGL(welch_partial_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, spec_x, spec_y, part, fstride, K,
                               sx.frames, c.ngroups, t0, g0, ng * K);
        else
            hipLaunchKernelGGL(welch_partial_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, spec_x, spec_y, part, fstride, K,
                               sx.frames, c.ngroups, t0, g0, ng * K);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        rc = launch_total(ctx, c, part, g0, ng);
        if (rc) return rc;
        t0 = end;
    }
    return KOFFT_OK;
}

static int welch_dev(kofft_hip_ctx *ctx, bool csd, const float *d_x, const float *d_y, size_t rows, size_t len, size_t row_stride,
              const float *d_window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_out)
{
    const int crc = welch_check(csd, d_x, d_y, d_window, d_out, rows, len, row_stride, win_len, hop, frames, flags, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    WelchCall c{};
    // A frame that begins at or past the end of its row is all +0: its terms are +-0 and change no sum (a sum seeded with +0 is never -0).
    // Only the frames that can hold a sample are walked, at least one, so that a row without samples still stores +0 * scale.
    const size_t holding = len ? (len - 1) / hop + 1 : 1;
    const int rc = framed_src(ctx, d_x, rows, len, row_stride, d_window, win_len, hop, frames < holding ? frames : holding, &c.src);
    if (rc) return rc;
    c.y = csd ? d_y : nullptr;
    c.ngroups = welch_groups(c.src.frames);
    c.scale = scale;
    c.twice = (flags & KOFFT_HIP_PSD_DOUBLE) ? 1 : 0;
    c.out = d_out;
    c.csd = csd;
    if (welch_use_fused(ctx, win_len)) return welch_fused(ctx, c);
    return welch_composed(ctx, c);
}

// The signals go up, rows * K values come down (whole rows per chunk of the pipeline); no frame leaves the device.
static int welch_host(kofft_hip_ctx *ctx, bool csd, const float *x, const float *y, size_t rows, size_t len, size_t row_stride,
                      const float *window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *out)
{
    const int crc = welch_check(csd, x, y, window, out, rows, len, row_stride, win_len, hop, frames, flags, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    const size_t out_row = (win_len / 2 + 1) * (csd ? 2 : 1);
    std::vector<float> packed_x, packed_y;
    const float *sx = pack_rows(x, rows, len, row_stride, packed_x);
    if (!csd)
        return rows_host<float>(ctx, sx, out, rows, len, out_row, window, window ? win_len : 0, true, true,
                                [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                    return welch_dev(ctx, false, d_in, nullptr, nb, len, len, d_win, win_len, hop, frames, scale, flags, d_out);
                                });
    const float *sy = pack_rows(y, rows, len, row_stride, packed_y);
    const HostArray<float> a[3] = {{sx, nullptr, len}, {sy, nullptr, len}, {nullptr, out, out_row}};
    return rows_host_n<float>(ctx, rows, 3, a, window, window ? win_len : 0, true, true, [&](float *const *d, const float *d_win, size_t nb) {
        return welch_dev(ctx, true, d[0], d[1], nb, len, len, d_win, win_len, hop, frames, scale, flags, d[2]);
    });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_welch_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                        size_t win_len, size_t hop, size_t frames, float scale, int flags, float *psd)
{
    return welch_host(ctx, false, signal, nullptr, rows, len, row_stride, window, win_len, hop, frames, scale, flags, psd);
}

int kofft_hip_dev_welch_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                            size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_psd)
{
    return welch_dev(ctx, false, d_signal, nullptr, rows, len, row_stride, d_window, win_len, hop, frames, scale, flags, d_psd);
}

int kofft_hip_csd_f32(kofft_hip_ctx *ctx, const float *x, const float *y, size_t rows, size_t len, size_t row_stride, const float *window,
                      size_t win_len, size_t hop, size_t frames, float scale, int flags, float *pxy)
{
    return welch_host(ctx, true, x, y, rows, len, row_stride, window, win_len, hop, frames, scale, flags, pxy);
}

int kofft_hip_dev_csd_f32(kofft_hip_ctx *ctx, const float *d_x, const float *d_y, size_t rows, size_t len, size_t row_stride,
                          const float *d_window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_pxy)
{
    return welch_dev(ctx, true, d_x, d_y, rows, len, row_stride, d_window, win_len, hop, frames, scale, flags, d_pxy);
}

int kofft_hip_set_welch_fused(kofft_hip_ctx *ctx, int mode) { return set_route(ctx, &kofft_hip_ctx::welch_fused, mode, 0, 2); }

int kofft_hip_welch_scale_f32(const float *window, size_t win_len, double fs, size_t frames, int scaling, float *scale)
{
    if (!scale) return KOFFT_ERR_NULL;
    if (win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if ((scaling != 0 && scaling != 1) || !(fs > 0.0) || frames == 0) return KOFFT_ERR_INVALID_VALUE;
    std::vector<float> hann;
    if (!window) {
        hann.resize(win_len);
        kofft_tables::hann_f32(win_len, hann.data());
        window = hann.data();
    }
    double s = 0.0;
    for (size_t i = 0; i < win_len; ++i) {
        const double w = (double)window[i];
        s = s + (scaling == 0 ? w * w : w);
    }
    const double den = scaling == 0 ? fs * s * (double)frames : (s * s) * (double)frames;
    if (s == 0.0 || !(den == den)) return KOFFT_ERR_INVALID_VALUE;
    *scale = (float)(1.0 / den);
    return KOFFT_OK;
}

}  // extern "C"
