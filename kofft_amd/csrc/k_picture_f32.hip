// k_picture_f32.hip -- rows of audio to spectrogram pictures in one call (picture_impl.hip.h): every kernel instance of
// the family, the argument checks and the routes of the three maximum modes.
#include "picture_impl.hip.h"
#include "host_stage.hip.h"

#include "frame_cut.h"

namespace kofft {
namespace host {

// the magnitudes kernels without stores run their parents' configurations
template <> struct PersistCfg<10, StftMagRowsMaxOnlyIO> : PersistCfg<10, StftMagIO> {};
template <> struct PersistCfg<11, StftMagRowsMaxOnlyIO> : PersistCfg<11, StftMagIO> {};
template <> struct PersistCfg<12, StftMagRowsMaxOnlyIO> : PersistCfg<12, StftMagIO> {};

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched.
static int picture_check(bool dev, const void *signal, size_t rows, size_t len, size_t row_stride, const void *window, size_t win_len, size_t hop,
                  size_t frames, int max_mode, const void *max_in, const void *max_out, int mode, int cmap, int depth, int channels, int scale,
                  int layout, const uint32_t *pix_of_bin, const void *out, const kofft_hip_ctx *ctx, bool *empty)
{
    *empty = false;
    // 1. the STFT rows'
    const int crc = stft_rows_check(true, true, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    // 2. the render's enums and its table
    const size_t bins = win_len / 2;
    if (mode < 0 || mode > 1 || scale < 0 || scale > 1 || layout < 0 || layout > 1 || (depth != 8 && depth != 16)) return KOFFT_ERR_INVALID_VALUE;
    if (cmap != KOFFT_CMAP_FIRE && cmap != KOFFT_CMAP_LEGACY && cmap != KOFFT_CMAP_GRAY && cmap != KOFFT_CMAP_RAINBOW)
        return KOFFT_ERR_INVALID_VALUE;  // unknown, or one of the colorous palettes
    if (scale == 1) {
        if (!pix_of_bin) return KOFFT_ERR_INVALID_VALUE;
        for (size_t b = 0; b < bins; ++b)
            if (pix_of_bin[b] >= bins) return KOFFT_ERR_INVALID_VALUE;
        for (size_t b = 1; b < bins; ++b)
            if (pix_of_bin[b] < pix_of_bin[b - 1]) return KOFFT_ERR_INVALID_VALUE;
    }
    // 3. this call's own
    if (max_mode < 0 || max_mode > 2 || (channels != 3 && channels != 4) || (channels == 4 && depth == 16) || (max_mode == 1 && scale == 1))
        return KOFFT_ERR_INVALID_VALUE;
    if (bins > kSpecMaxBins) return KOFFT_ERR_UNSUPPORTED;  // (the picture's bytes fit a size_t: rows * frames * win_len <= SIZE_MAX / 16)
    // 4. no bins: only max_out is written
    if (win_len == 1) {
        *empty = true;
        return KOFFT_OK;
    }
    // 5. null pointers
    if (!ctx || !out || (!signal && len) || (max_mode == 2 && !max_in)) return KOFFT_ERR_NULL;
    // 6. (device forms) the output against every input and against max_out
    if (dev) {
        const size_t px = channels == 4 ? 4 : (depth == 16 ? 6 : 3);
        const size_t out_bytes = rows * frames * bins * px;
        if (overlaps(out, out_bytes, signal, rows_span(rows, len, row_stride) * sizeof(float)) || overlaps(out, out_bytes, window, win_len * sizeof(float)) ||
            (max_mode == 2 && overlaps(out, out_bytes, max_in, rows * sizeof(float))) || overlaps(out, out_bytes, max_out, rows * sizeof(float)))
            return KOFFT_ERR_INVALID_VALUE;
    }
    return KOFFT_OK;
}

static unsigned pic_blocks(const kofft_hip_ctx *ctx, size_t items)
{
    const size_t need = (items + 255) / 256, cap = (size_t)ctx->num_cus * 32;
    return (unsigned)(need < cap ? need : cap);
}

// what one call works with
struct PicCall {
    kofft_hip_ctx *ctx;
    FramedSrc src;
    size_t half;  // src.win_len / 2
    float *mags, *pmax, *fmax;
    cpx<float> *spec;
    const float *row_max;  // the maximum the render reads per row (modes 0 and 2)
    int mode, cmap, fmt, layout;
    float level;
    const uint32_t *start;
    unsigned char *out;
};

// magnitudes of frames [t0, t0 + nt) of the flat index, dense at c.mags
static int pic_produce(const PicCall &c, size_t t0, size_t nt) { return framed_produce(c.ctx, c.src, FRAMES_MAGS, t0, nt, c.mags, c.spec); }

template <int FMT, bool PMAX>
static int pic_render_as(const PicCall &c, size_t t0, size_t nt)
{
    kofft_hip_ctx *ctx = c.ctx;
    constexpr size_t PX = pic_px(FMT);
    const int bins = (int)c.half;
    const size_t frames = c.src.frames;
    if (c.layout == 0) {
        hipLaunchKernelGGL((pic_flat_kernel<FMT, PMAX>), dim3(pic_blocks(ctx, (nt * c.half + 3) / 4)), dim3(256), 0, ctx->stream, c.mags, c.pmax,
                           c.out + t0 * c.half * PX, nt, bins, c.row_max, t0 / frames, (t0 % frames) * c.half, frames * c.half, c.mode, c.level, c.cmap,
                           c.start);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return KOFFT_OK;
    }
    FramePiece p[3];
    const int np = frame_cut(t0, nt, frames, p);
    for (int k = 0; k < np; ++k) {
        const size_t tiles_b = (c.half + SPEC_TB - 1) / SPEC_TB, tiles_f = (p[k].nf + SPEC_TF - 1) / SPEC_TF;
        if (tiles_f > 0x7fffffffULL / tiles_b || p[k].nr > 0x7fffffffULL / (tiles_b * tiles_f)) return KOFFT_ERR_UNSUPPORTED;
        auto kern = ctx->spec_transpose ? pic_image_kernel<FMT, true, PMAX> : pic_image_kernel<FMT, false, PMAX>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_b * tiles_f * p[k].nr)), dim3(SPEC_THREADS), 0, ctx->stream, c.mags + p[k].at * c.half,
                           PMAX ? c.pmax + p[k].at * c.half : nullptr, c.out, p[k].row, p[k].f0, p[k].nf, frames, bins, c.row_max, c.mode,
                           c.level, c.cmap, c.start, (unsigned)tiles_b, (unsigned)tiles_f);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

static int pic_render(const PicCall &c, bool per_pixel, size_t t0, size_t nt)
{
    switch (c.fmt) {
    case 0: return per_pixel ? pic_render_as<0, true>(c, t0, nt) : pic_render_as<0, false>(c, t0, nt);
    case 1: return per_pixel ? pic_render_as<1, true>(c, t0, nt) : pic_render_as<1, false>(c, t0, nt);
    default: return per_pixel ? pic_render_as<2, true>(c, t0, nt) : pic_render_as<2, false>(c, t0, nt);
    }
}

// the row maxima of the chunk at c.mags into max_bits
static int pic_row_max(const PicCall &c, unsigned *max_bits, size_t t0, size_t nt)
{
    hipLaunchKernelGGL(pic_row_max_kernel, dim3(pic_blocks(c.ctx, nt * c.half)), dim3(256), 0, c.ctx->stream, c.mags, max_bits, c.src.frames, c.half, t0,
                       nt * c.half);
    KOFFT_HIP_TRY(c.ctx, hipGetLastError());
    return KOFFT_OK;
}

// the running maximum of the chunk at c.mags: c.fmax (per frame, exclusive over the row's earlier frames), then c.pmax (per pixel)
static int pic_running(const PicCall &c, float *carry, size_t t0, size_t nt)
{
    kofft_hip_ctx *ctx = c.ctx;
    const unsigned per_frame = (unsigned)((nt + 3) / 4);  // (nt <= 2^27: a chunk holds at most 2^27 floats)
    hipLaunchKernelGGL(pic_frame_max_kernel, dim3(per_frame), dim3(256), 0, ctx->stream, c.mags, c.fmax, nt, (int)c.half);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    const size_t nrows = (t0 + nt - 1) / c.src.frames - t0 / c.src.frames + 1;
    if (nrows > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pic_frame_scan_kernel, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, c.fmax, carry, c.src.frames, t0, nt);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pic_pixel_max_kernel, dim3(per_frame), dim3(256), 0, ctx->stream, c.mags, c.fmax, c.pmax, nt, (int)c.half);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

static int pic_fill(kofft_hip_ctx *ctx, float *dst, size_t count, float value)
{
    const size_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pic_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, dst, count, value);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

static size_t pad16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dev_stft_picture_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                   const float *d_window, size_t win_len, size_t hop, size_t frames, int max_mode, const float *d_max_in,
                                   float *d_max_out, int mode, float level, int cmap, int depth, int channels, int scale, int layout,
                                   const uint32_t *pix_of_bin, void *d_out)
{
    bool empty = false;
    int rc = picture_check(true, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, max_mode, d_max_in, d_max_out, mode, cmap, depth,
                           channels, scale, layout, pix_of_bin, d_out, ctx, &empty);
    if (rc || rows == 0 || frames == 0) return rc;
    if (empty) {  // every maximum is its starting value; the context is needed only where there is something to write
        if (max_mode == 2 && !d_max_in) return KOFFT_ERR_NULL;
        if (!d_max_out) return KOFFT_OK;
        if (!ctx) return KOFFT_ERR_NULL;
        KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (max_mode == 2) {
            if (d_max_out != d_max_in) KOFFT_HIP_TRY(ctx, hipMemcpyAsync(d_max_out, d_max_in, rows * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            return KOFFT_OK;
        }
        return pic_fill(ctx, d_max_out, rows, max_mode == 1 ? kPicSeed : 0.0f);
    }
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    PicCall c{};
    c.ctx = ctx;
    rc = framed_src(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, &c.src);
    if (rc) return rc;
    c.half = win_len / 2;
    c.mode = mode, c.level = level, c.cmap = cmap, c.layout = layout;
    c.fmt = channels == 4 ? 2 : (depth == 16 ? 1 : 0);
    c.out = static_cast<unsigned char *>(d_out);
    if (scale == 1) {
        rc = get_spec_ranges(ctx, pix_of_bin, c.half, &c.start);
        if (rc) return rc;
    }

    // scratch: [magnitudes | (mode 1) the per-pixel maxima | (composed window lengths) the frames | a float per row | (mode 1) a float per frame]
    const size_t total = rows * frames;
    const bool running = max_mode == 1;
    const size_t frame_bytes = c.half * sizeof(float) * (running ? 2 : 1) + (c.src.kernels ? 0 : win_len * sizeof(cpx<float>));
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, frame_bytes, total);
    const size_t mags_bytes = pad16(chunk * c.half * sizeof(float));
    const size_t spec_bytes = c.src.kernels ? 0 : pad16(chunk * win_len * sizeof(cpx<float>));
    const size_t per_row_bytes = pad16(rows * sizeof(float));
    rc = ensure(ctx, ctx->rows_tmp, mags_bytes * (running ? 2 : 1) + spec_bytes + per_row_bytes + (running ? pad16(chunk * sizeof(float)) : 0) + 16);
    if (rc) return rc;
    char *base = static_cast<char *>(ctx->rows_tmp.p);
    c.mags = reinterpret_cast<float *>(base);
    base += mags_bytes;
    if (running) {
        c.pmax = reinterpret_cast<float *>(base);
        base += mags_bytes;
    }
    c.spec = reinterpret_cast<cpx<float> *>(base);
    base += spec_bytes;
    float *per_row = reinterpret_cast<float *>(base);  // mode 0: the row maxima; mode 1: the carries
    base += per_row_bytes;
    c.fmax = reinterpret_cast<float *>(base);

    if (max_mode == 2) {
        c.row_max = d_max_in;
        rc = for_chunks(total, chunk, [&](size_t t0, size_t nt) {
            const int prc = pic_produce(c, t0, nt);
            return prc ? prc : pic_render(c, false, t0, nt);
        });
        if (rc) return rc;
        if (d_max_out && d_max_out != d_max_in)
            KOFFT_HIP_TRY(ctx, hipMemcpyAsync(d_max_out, d_max_in, rows * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return KOFFT_OK;
    }

    if (running) {
        rc = pic_fill(ctx, per_row, rows, kPicSeed);
        if (rc) return rc;
        rc = for_chunks(total, chunk, [&](size_t t0, size_t nt) {
            int prc = pic_produce(c, t0, nt);
            if (!prc) prc = pic_running(c, per_row, t0, nt);
            return prc ? prc : pic_render(c, true, t0, nt);
        });
    } else {
        c.row_max = per_row;
        unsigned *max_bits = reinterpret_cast<unsigned *>(per_row);
        if (chunk == total && !d_window) {
            // everything fits one chunk: the chain's own kernels, the maximum riding on the magnitudes' stores
            rc = stft_mag_rows_dev(ctx, d_signal, rows, len, row_stride, win_len, hop, c.mags, frames, per_row);
            if (!rc) rc = pic_render(c, false, 0, total);
        } else {
            KOFFT_HIP_TRY(ctx, hipMemsetAsync(per_row, 0, rows * sizeof(float), ctx->stream));  // every maximum starts at +0
            if (chunk == total) {  // a caller's window: the maximum from the magnitudes in scratch
                rc = pic_produce(c, 0, total);
                if (!rc) rc = pic_row_max(c, max_bits, 0, total);
                if (!rc) rc = pic_render(c, false, 0, total);
            } else {
                // two passes.  The first keeps nothing but the maxima: the magnitudes kernels without their stores over the whole batch,
                // or (composed window lengths) chunk after chunk through the scratch
                if (c.src.kernels) {
                    StftMagRowsMaxOnlyIO io{};
                    fill_rows_io(io, c.src);
                    io.mags = nullptr;
                    io.max_bits = max_bits;
                    rc = dispatch<float, EPI_STORE>(ctx, io, win_len, total);
                } else {
                    rc = for_chunks(total, chunk, [&](size_t t0, size_t nt) {
                        const int prc = pic_produce(c, t0, nt);
                        return prc ? prc : pic_row_max(c, max_bits, t0, nt);
                    });
                }
                if (!rc)
                    rc = for_chunks(total, chunk, [&](size_t t0, size_t nt) {
                        const int prc = pic_produce(c, t0, nt);
                        return prc ? prc : pic_render(c, false, t0, nt);
                    });
            }
        }
    }
    if (rc) return rc;
    if (d_max_out) KOFFT_HIP_TRY(ctx, hipMemcpyAsync(d_max_out, per_row, rows * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return KOFFT_OK;
}


// The signal (and mode 2's maxima) go up, the pictures and the maxima come down, all as bytes, whole rows per chunk of the pipeline: a
// row's running maximum never crosses a chunk of the pipeline.  Never zero-copy: the maxima are atomicMax targets and stay in device memory.
int kofft_hip_stft_picture_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                               size_t win_len, size_t hop, size_t frames, int max_mode, const float *max_in, float *max_out, int mode,
                               float level, int cmap, int depth, int channels, int scale, int layout, const uint32_t *pix_of_bin, void *out)
{
    bool empty = false;
    const int crc = picture_check(false, signal, rows, len, row_stride, window, win_len, hop, frames, max_mode, max_in, max_out, mode, cmap,
                                  depth, channels, scale, layout, pix_of_bin, out, ctx, &empty);
    if (crc || rows == 0 || frames == 0) return crc;
    if (empty) {
        if (max_mode == 2 && !max_in) return KOFFT_ERR_NULL;
        for (size_t r = 0; max_out && r < rows; ++r) max_out[r] = max_mode == 2 ? max_in[r] : (max_mode == 1 ? 1e-12f : 0.0f);
        return KOFFT_OK;
    }
    typedef unsigned char byte;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    const size_t px = channels == 4 ? 4 : (depth == 16 ? 6 : 3);
    const HostArray<byte> a[4] = {{reinterpret_cast<const byte *>(src), nullptr, len * sizeof(float)},
                                  {nullptr, static_cast<byte *>(out), frames * (win_len / 2) * px},
                                  {max_mode == 2 ? reinterpret_cast<const byte *>(max_in) : nullptr, nullptr, sizeof(float)},
                                  {nullptr, reinterpret_cast<byte *>(max_out), sizeof(float)}};
    return rows_host_n<byte>(ctx, rows, 4, a, reinterpret_cast<const byte *>(window), window ? win_len * sizeof(float) : 0, false, true,
                             [&](byte *const *d, const byte *d_win, size_t nb) {
                                 return kofft_hip_dev_stft_picture_f32(
                                     ctx, reinterpret_cast<const float *>(d[0]), nb, len, len, reinterpret_cast<const float *>(d_win), win_len, hop,
                                     frames, max_mode, max_mode == 2 ? reinterpret_cast<const float *>(d[2]) : nullptr,
                                     max_out ? reinterpret_cast<float *>(d[3]) : nullptr, mode, level, cmap, depth, channels, scale, layout,
                                     pix_of_bin, d[1]);
                             });
}

}  // extern "C"
