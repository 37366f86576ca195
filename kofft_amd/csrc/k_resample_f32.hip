// k_resample_f32.hip -- polyphase resampling of float rows (resample_impl.hip.h): the two kernels, the argument
// checks, the extern "C" entry points and the host-only tap design.
#include "resample_impl.hip.h"
#include "host_stage.hip.h"
#include "kaiser_i0.h"

#include <cmath>
#include <new>
#include <vector>

namespace kofft {
namespace host {

static_assert(kResampleTile == KOFFT_HIP_RESAMPLE_TILE, "include/kofft_hip.h names the tile");

// The argument checks alone, in the order of include/kofft_hip.h and before the context or a device is touched.  KOFFT_OK with
// rows == 0 or out_len == 0: nothing to do.
static int resample_check(size_t rows, size_t nx, size_t nh, size_t up, size_t down, size_t t0, size_t out_len, const void *x, const void *h,
                   const void *out, const kofft_hip_ctx *ctx)
{
    if (rows == 0 || out_len == 0) return KOFFT_OK;
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (up == 0 || down == 0) return KOFFT_ERR_INVALID_VALUE;
    size_t full_up = 0, last = 0, in_bytes = 0, out_bytes = 0, h_bytes = 0;
    if (__builtin_mul_overflow(nx - 1, up, &full_up) || __builtin_add_overflow(full_up, nh, &full_up)) return KOFFT_ERR_UNSUPPORTED;
    if (__builtin_mul_overflow(out_len - 1, down, &last) || __builtin_add_overflow(last, t0, &last)) return KOFFT_ERR_UNSUPPORTED;
    if (__builtin_mul_overflow(rows, nx, &in_bytes) || __builtin_mul_overflow(in_bytes, sizeof(float), &in_bytes) ||
        __builtin_mul_overflow(rows, out_len, &out_bytes) || __builtin_mul_overflow(out_bytes, sizeof(float), &out_bytes) ||
        __builtin_mul_overflow(nh, sizeof(float), &h_bytes))
        return KOFFT_ERR_UNSUPPORTED;
    if (last >= full_up) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (!ctx || !x || !h || !out) return KOFFT_ERR_NULL;
    if (overlaps(out, out_bytes, x, in_bytes) || overlaps(out, out_bytes, h, h_bytes)) return KOFFT_ERR_INVALID_VALUE;
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dev_resample_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t nh, size_t up,
                               size_t down, size_t t0, float *d_out, size_t out_len)
{
    const int crc = resample_check(rows, nx, nh, up, down, t0, out_len, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ResampleShape s{};
    s.nx = nx;
    s.nh = nh;
    s.up = up;
    s.down = down;
    s.t0 = t0;
    s.out_len = out_len;
    s.terms = resample_max_terms(nh, up);
    s.tap_stride = resample_tap_stride(s.terms);
    s.lanes = resample_phase_lanes(up, down);
    s.tile = resample_tile_outputs(up, down);
    s.tiles_per_row = out_len / s.tile + (out_len % s.tile != 0);
    s.total = rows * out_len;
    const bool tiled = ctx->resample_tiled == 2 ? resample_fits(nh, up, down) : ctx->resample_tiled == 1 && resample_route(nh, up, down) == 1;
    if (tiled && !__builtin_mul_overflow(rows, s.tiles_per_row, &s.ntiles)) {
        const size_t cap = (size_t)ctx->num_cus * 32;
        const size_t lds = (size_t)resample_lds_words(nh, up, down, kResampleTile) * sizeof(float);  // at most 52 KiB: no attribute
        const dim3 grid((unsigned)(s.ntiles < cap ? s.ntiles : cap));
        if (s.lanes)
            hipLaunchKernelGGL(resample_tiled_kernel<true>, grid, dim3(kResampleThreads), lds, ctx->stream, d_x, d_h, d_out, s);
        else
            hipLaunchKernelGGL(resample_tiled_kernel<false>, grid, dim3(kResampleThreads), lds, ctx->stream, d_x, d_h, d_out, s);
    } else {
        const size_t want = (s.total + kResampleThreads - 1) / kResampleThreads, cap = (size_t)ctx->num_cus * 64;
        hipLaunchKernelGGL(resample_plain_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(kResampleThreads), 0, ctx->stream, d_x, d_h,
                           d_out, s);
    }
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// nx samples per row go up, out_len values come down; the one filter is the side input, uploaded once
int kofft_hip_resample_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t nh, size_t up, size_t down,
                           size_t t0, float *out, size_t out_len)
{
    const int crc = resample_check(rows, nx, nh, up, down, t0, out_len, x, h, out, ctx);
    if (crc || rows == 0 || out_len == 0) return crc;
    return rows_host<float>(ctx, x, out, rows, nx, out_len, h, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return kofft_hip_dev_resample_f32(ctx, d_in, nr, nx, d_h, nh, up, down, t0, d_out, out_len);
                            });
}

int kofft_hip_set_resample_tiled(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::resample_tiled, on, 0, 2); }

int kofft_hip_resample_route(size_t nh, size_t up, size_t down, int *route)
{
    if (!route) return KOFFT_ERR_NULL;
    if (nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (up == 0 || down == 0) return KOFFT_ERR_INVALID_VALUE;
    *route = resample_route(nh, up, down);
    return KOFFT_OK;
}

// scipy.signal.resample_poly's default filter: firwin(2 * half + 1, 1 / max(up, down), window = ("kaiser", beta)) * up with
// half = zeros * max(up, down) -- the sinc of that cutoff under a Kaiser window, normalised to unit sum, times up; double throughout
// and rounded to f32 once.
int kofft_hip_resample_taps_f32(size_t up, size_t down, size_t zeros, double beta, float *taps, size_t *nh_out)
{
    if (!taps && !nh_out) return KOFFT_ERR_NULL;
    if (up == 0 || down == 0 || zeros == 0 || !(beta >= 0.0)) return KOFFT_ERR_INVALID_VALUE;
    const size_t mx = up > down ? up : down;
    size_t half = 0, nh = 0;
    if (__builtin_mul_overflow(zeros, mx, &half) || __builtin_mul_overflow(half, (size_t)2, &nh) || __builtin_add_overflow(nh, (size_t)1, &nh))
        return KOFFT_ERR_UNSUPPORTED;
    if (nh_out) *nh_out = nh;
    if (!taps) return KOFFT_OK;
    if (nh > (size_t(1) << 28)) return KOFFT_ERR_UNSUPPORTED;
    std::vector<double> h;
    try {
        h.resize(nh);
    } catch (const std::bad_alloc &) {
        return KOFFT_ERR_ALLOC;
    }
    const double cutoff = 1.0 / (double)mx, alpha = (double)half, i0b = bessel_i0(beta);
    double sum = 0.0;
    for (size_t n = 0; n < nh; ++n) {
        const double m = (double)n - alpha;
        const double y = M_PI * (cutoff * m);
        const double sinc = y == 0.0 ? 1.0 : std::sin(y) / y;
        const double r = m / alpha, inside = 1.0 - r * r;
        const double w = bessel_i0(beta * std::sqrt(inside > 0.0 ? inside : 0.0)) / i0b;
        h[n] = (cutoff * sinc) * w;
        sum = sum + h[n];
    }
    for (size_t n = 0; n < nh; ++n) taps[n] = (float)(h[n] / sum * (double)up);
    return KOFFT_OK;
}

}  // extern "C"
