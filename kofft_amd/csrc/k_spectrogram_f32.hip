// k_spectrogram_f32.hip -- visual::spectrogram's colour helpers (spectrogram.rs:96-234) on float magnitudes: every kernel instance of
// the family (spectrogram_impl.hip.h), the argument checks, the per-context cache of pixel ranges and the host's map_color_u8.
#include "spectrogram_impl.hip.h"
#include "host_stage.hip.h"

#include <algorithm>

namespace kofft {
namespace host {

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched.
static int spec_db_check(bool dev, const void *mags, size_t count, const void *max_mag, const void *out, const kofft_hip_ctx *ctx)
{
    if (count == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (count > SIZE_MAX / sizeof(float)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !mags || !max_mag || !out) return KOFFT_ERR_NULL;
    if (dev && (overlaps(mags, count * sizeof(float), out, count * sizeof(float)) || overlaps(max_mag, sizeof(float), out, count * sizeof(float))))
        return KOFFT_ERR_INVALID_VALUE;
    return KOFFT_OK;
}

static int spec_render_check(bool dev, const void *mags, size_t frames, size_t bins, const void *max_mag, int mode, int cmap, int depth, int scale,
                      int layout, const uint32_t *pix_of_bin, const void *out, const kofft_hip_ctx *ctx)
{
    if (frames == 0 || bins == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (mode < 0 || mode > 1 || scale < 0 || scale > 1 || layout < 0 || layout > 1 || (depth != 8 && depth != 16)) return KOFFT_ERR_INVALID_VALUE;
    if (cmap != KOFFT_CMAP_FIRE && cmap != KOFFT_CMAP_LEGACY && cmap != KOFFT_CMAP_GRAY && cmap != KOFFT_CMAP_RAINBOW)
        return KOFFT_ERR_INVALID_VALUE;  // unknown, or one of the colorous palettes
    if (scale == 1) {
        if (!pix_of_bin) return KOFFT_ERR_INVALID_VALUE;
        for (size_t b = 0; b < bins; ++b)
            if (pix_of_bin[b] >= bins) return KOFFT_ERR_INVALID_VALUE;
        for (size_t b = 1; b < bins; ++b)
            if (pix_of_bin[b] < pix_of_bin[b - 1]) return KOFFT_ERR_INVALID_VALUE;  // its pixels are not ranges of bins
    }
    const size_t px = depth == 16 ? 6 : 3;
    if (bins > kSpecMaxBins || frames > SIZE_MAX / (bins * px)) return KOFFT_ERR_UNSUPPORTED;
    const size_t tiles_b = (bins + SPEC_TB - 1) / SPEC_TB, tiles_f = (frames + SPEC_TF - 1) / SPEC_TF;
    if (tiles_f > 0x7fffffffULL / tiles_b) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !mags || !max_mag || !out) return KOFFT_ERR_NULL;
    const size_t in_bytes = frames * bins * sizeof(float), out_bytes = frames * bins * px;
    if (dev && (overlaps(mags, in_bytes, out, out_bytes) || overlaps(max_mag, sizeof(float), out, out_bytes))) return KOFFT_ERR_INVALID_VALUE;
    return KOFFT_OK;
}

void spec_drop(kofft_hip_ctx *ctx)
{
    for (auto &slot : ctx->spec_slots)
        if (slot.d_start) (void)hipFree(slot.d_start);
    ctx->spec_slots.clear();
}

// The device ranges of a (checked) table: a hit moves its slot to the front; a miss builds the ranges on the host, uploads them on the
// context's stream (from the slot's own staging vector, which outlives the copy) and, with kSpecSlots tables already there, frees the
// least recently used one after a stream synchronisation.
int get_spec_ranges(kofft_hip_ctx *ctx, const uint32_t *pix_of_bin, size_t bins, const uint32_t **out)
{
    auto &slots = ctx->spec_slots;
    for (size_t j = 0; j < slots.size(); ++j) {
        if (slots[j].table.size() == bins && std::memcmp(slots[j].table.data(), pix_of_bin, bins * sizeof(uint32_t)) == 0) {
            if (j) std::rotate(slots.begin(), slots.begin() + j, slots.begin() + j + 1);
            *out = static_cast<const uint32_t *>(slots[0].d_start);
            return KOFFT_OK;
        }
    }
    try {
        kofft_spec_slot slot;
        slot.table.assign(pix_of_bin, pix_of_bin + bins);
        slot.staged.resize(bins + 1);
        if (!kofft_tables::spec_ranges_build(pix_of_bin, bins, slot.staged.data())) return KOFFT_ERR_INVALID_VALUE;
        if (slots.size() >= kSpecSlots) {
            KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (slots.back().d_start) (void)hipFree(slots.back().d_start);
            slots.pop_back();
        }
        if (const char *bad = HipAlloc::alloc(&slot.d_start, slot.staged.size() * sizeof(uint32_t)))
            return report_failure(ctx, KOFFT_ERR_HIP, "spectrogram ranges: allocation", bad);
        slots.insert(slots.begin(), std::move(slot));
    } catch (const std::bad_alloc &) {
        return report_failure(ctx, KOFFT_ERR_ALLOC, "spectrogram ranges", "out of host memory");
    }
    kofft_spec_slot &s = slots.front();
    const hipError_t e = hipMemcpyAsync(s.d_start, s.staged.data(), s.staged.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s.d_start);
        slots.erase(slots.begin());
        return report_failure(ctx, KOFFT_ERR_HIP, "spectrogram ranges: upload", hipGetErrorString(e));
    }
    *out = static_cast<const uint32_t *>(s.d_start);
    return KOFFT_OK;
}

static int spec_db_dev(kofft_hip_ctx *ctx, int which, const float *d_mags, size_t count, const float *d_max, float level, float *d_out)
{
    const int rc = spec_db_check(true, d_mags, count, d_max, d_out, ctx);
    if (rc) return rc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spec_db_kernel, dim3(flat_blocks(ctx, count, 32)), dim3(256), 0, ctx->stream, d_mags, d_out, count, d_max, level, which);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// magnitude_to_db (which == 0) / db_scale on `count` host magnitudes, max_mag a host float: one row of `count` values with max_mag as
// the side input
static int spec_db_host(kofft_hip_ctx *ctx, int which, const float *mags, size_t count, const float *max_mag, float level, float *out)
{
    const int crc = spec_db_check(false, mags, count, max_mag, out, ctx);
    if (crc) return crc;
    return rows_host<float>(ctx, mags, out, 1, count, count, max_mag, 1, true, true,
                            [&](float *d_in, float *d_out, const float *d_max, size_t) { return spec_db_dev(ctx, which, d_in, count, d_max, level, d_out); });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float floor_db, float *out)
{
    return spec_db_host(ctx, 0, mags, count, max_mag, floor_db, out);
}
int kofft_hip_dev_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float floor_db,
                                      float *d_out)
{
    return spec_db_dev(ctx, 0, d_mags, count, d_max_mag, floor_db, d_out);
}
int kofft_hip_db_scale_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float dynamic_range, float *out)
{
    return spec_db_host(ctx, 1, mags, count, max_mag, dynamic_range, out);
}
int kofft_hip_dev_db_scale_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float dynamic_range,
                               float *d_out)
{
    return spec_db_dev(ctx, 1, d_mags, count, d_max_mag, dynamic_range, d_out);
}

int kofft_hip_set_spectrogram_transpose(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::spec_transpose, on); }

int kofft_hip_log_bin_map(size_t bins, uint32_t *pix_of_bin)
{
    if (bins == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (bins > kSpecMaxBins) return KOFFT_ERR_UNSUPPORTED;
    if (!pix_of_bin) return KOFFT_ERR_NULL;
    kofft_tables::log_bin_map(bins, pix_of_bin);
    return KOFFT_OK;
}

int kofft_hip_dev_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t frames, size_t bins, const float *d_max, int mode,
                                         float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin, void *d_out)
{
    int rc = spec_render_check(true, d_mags, frames, bins, d_max, mode, cmap, depth, scale, layout, pix_of_bin, d_out, ctx);
    if (rc) return rc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t *start = nullptr;
    if (scale == 1) {
        rc = get_spec_ranges(ctx, pix_of_bin, bins, &start);
        if (rc) return rc;
    }
    unsigned char *out = static_cast<unsigned char *>(d_out);
    const bool d16 = depth == 16;
    if (layout == 0) {
        auto kern = d16 ? spec_flat_kernel<true> : spec_flat_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(flat_blocks(ctx, (frames * bins + 3) / 4, 32)), dim3(256), 0, ctx->stream, d_mags, out, frames, (int)bins,
                           d_max, mode, level, cmap, start);
    } else {
        const size_t tiles_b = (bins + SPEC_TB - 1) / SPEC_TB, tiles_f = (frames + SPEC_TF - 1) / SPEC_TF;
        auto kern = ctx->spec_transpose ? (d16 ? spec_image_kernel<true, true> : spec_image_kernel<false, true>)
                                        : (d16 ? spec_image_kernel<true, false> : spec_image_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_b * tiles_f)), dim3(SPEC_THREADS), 0, ctx->stream, d_mags, out, frames, (int)bins, d_max,
                           mode, level, cmap, start, (unsigned)tiles_b);
    }
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// the render on a host picture: the magnitudes and the picture travel as bytes (one row each), max_mag as the side input; the table
// stays on the host
int kofft_hip_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *mags, size_t frames, size_t bins, const float *max_mag, int mode,
                                     float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin, void *out)
{
    const int crc = spec_render_check(false, mags, frames, bins, max_mag, mode, cmap, depth, scale, layout, pix_of_bin, out, ctx);
    if (crc) return crc;
    typedef unsigned char byte;
    return rows_host<byte>(ctx, reinterpret_cast<const byte *>(mags), static_cast<byte *>(out), 1, frames * bins * sizeof(float),
                           frames * bins * (depth == 16 ? 6 : 3), reinterpret_cast<const byte *>(max_mag), sizeof(float), true, true,
                           [&](byte *d_in, byte *d_out, const byte *d_max, size_t) {
                               return kofft_hip_dev_spectrogram_render_f32(ctx, reinterpret_cast<const float *>(d_in), frames, bins,
                                                                           reinterpret_cast<const float *>(d_max), mode, level, cmap, depth, scale,
                                                                           layout, pix_of_bin, d_out);
                           });
}

int kofft_hip_map_color_u8(float t, int cmap, unsigned char *rgb)
{
    if (cmap != KOFFT_CMAP_FIRE && cmap != KOFFT_CMAP_LEGACY && cmap != KOFFT_CMAP_GRAY && cmap != KOFFT_CMAP_RAINBOW) return KOFFT_ERR_INVALID_VALUE;
    if (!rgb) return KOFFT_ERR_NULL;
    const uint32_t c = spec_map_color(t, cmap);
    rgb[0] = (unsigned char)(c & 255u);
    rgb[1] = (unsigned char)((c >> 8) & 255u);
    rgb[2] = (unsigned char)((c >> 16) & 255u);
    return KOFFT_OK;
}

}  // extern "C"
