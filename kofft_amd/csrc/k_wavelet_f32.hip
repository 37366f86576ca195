// k_wavelet_f32.hip -- wavelet::* (wavelet.rs) on float rows: the argument checks, the routes, every kernel instance of the
// family (wavelet_impl.hip.h) and the extern "C" entry points.
#include "wavelet_impl.hip.h"
#include "host_stage.hip.h"

#include <atomic>
#include <type_traits>

namespace kofft {
namespace host {

using namespace kofft::wav;

constexpr size_t kWaveletMaxLen = size_t(1) << 26;  // the longest input or output row
constexpr size_t kWaveletMaxLevels = 64;
constexpr size_t kWaveletFusedMax = 16384;  // the longest row (forward: input, inverse: output) the fused multi-level kernels keep in LDS

namespace {

template <class Fn>
int dispatch(int w, Fn fn)
{
    switch (w) {
    case HAAR: return fn(std::integral_constant<int, HAAR>());
    case DB2: return fn(std::integral_constant<int, DB2>());
    case DB4: return fn(std::integral_constant<int, DB4>());
    case SYM4: return fn(std::integral_constant<int, SYM4>());
    case COIF1: return fn(std::integral_constant<int, COIF1>());
    default: return KOFFT_ERR_INVALID_VALUE;
    }
}

// any two of the ranges (pointer, bytes) overlap
bool any_overlap(std::initializer_list<std::pair<const void *, size_t>> r)
{
    for (auto i = r.begin(); i != r.end(); ++i)
        for (auto j = i + 1; j != r.end(); ++j)
            if (overlaps(i->first, i->second, j->first, j->second)) return true;
    return false;
}

// one level forward: rows of c samples reflected over lp (n = lp / 2 outputs)
template <int W>
int launch_fwd(kofft_hip_ctx *ctx, const float *x, float *a, float *d, size_t c, size_t lp, size_t rows)
{
    const size_t n = lp / 2;
    if (n == 0 || rows == 0) return KOFFT_OK;
    const int rpt = n <= (size_t)WV_TILE / 2 ? (int)(WV_TILE / n) : 1;
    const unsigned tiles = rpt > 1 ? 1u : (unsigned)((n + WV_TILE - 1) / WV_TILE);
    const size_t groups = (rows + rpt - 1) / rpt;
    const dim3 grid(tiles, (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(wavelet_fwd_kernel<W>, grid, dim3(WV_BLOCK), 0, ctx->stream, x, a, d, (int)c, (int)lp, rows, rpt);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// one level inverse: rows of c approximations and details (detail stride ds) to rows of 2c
template <int W>
int launch_inv(kofft_hip_ctx *ctx, const float *a, const float *d, float *out, size_t c, size_t ds, size_t rows)
{
    if (c == 0 || rows == 0) return KOFFT_OK;
    const int rpt = c <= (size_t)WV_TILE / 2 ? (int)(WV_TILE / c) : 1;
    const unsigned tiles = rpt > 1 ? 1u : (unsigned)((c + WV_TILE - 1) / WV_TILE);
    const size_t groups = (rows + rpt - 1) / rpt;
    const dim3 grid(tiles, (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(wavelet_inv_kernel<W>, grid, dim3(WV_BLOCK), 0, ctx->stream, a, d, out, (int)c, (int)ds, rows, rpt);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// rows per workgroup of the fused kernels: whole rows up to kWaveletPackFloats floats of input (forward) / output (inverse)
constexpr size_t kWaveletPackFloats = 8192;
constexpr size_t kMaxBlocks = size_t(1) << 30;

template <int W>
int launch_fwd_fused(kofft_hip_ctx *ctx, const float *x, float *approx, float *det, size_t len, size_t levels, size_t rows)
{
    static std::atomic<unsigned long long> lds_set{0};
    size_t rpb = len < kWaveletPackFloats ? kWaveletPackFloats / len : 1;
    if (rpb > rows) rpb = rows;
    const size_t bufa = (rpb * len + 3) & ~size_t(3);
    const size_t lds = (bufa + rpb * ((len + 1) / 2)) * sizeof(float);
    // The LDS grows with the row past kWaveletPackFloats (one row per workgroup: 72000 bytes at 12000 samples, 98304 at 16384), but the
    // attribute is set once per process: it is set to the largest this kernel takes, the kWaveletFusedMax-sample row, whatever row
    // length comes first.  (Shorter rows pack rpb rows into at most kWaveletPackFloats + kWaveletPackFloats floats: 64 KiB.)
    constexpr size_t kMaxLds = (((kWaveletFusedMax + 3) & ~size_t(3)) + (kWaveletFusedMax + 1) / 2) * sizeof(float);
    static_assert(kMaxLds >= 2 * kWaveletPackFloats * sizeof(float) && kMaxLds <= 160 * 1024, "fused forward LDS");
    if (lds > kMaxLds) return KOFFT_ERR_UNSUPPORTED;  // (never: len <= kWaveletFusedMax, use_fused)
    if (lds > (size_t(64) << 10)) {
        const int rc = set_dyn_lds_once(ctx, lds_set, reinterpret_cast<const void *>(wavelet_fwd_fused_kernel<W>), kMaxLds);
        if (rc) return rc;
    }
    const size_t blocks = (rows + rpb - 1) / rpb;
    for (size_t b0 = 0; b0 < blocks; b0 += kMaxBlocks) {
        const size_t nb = blocks - b0 < kMaxBlocks ? blocks - b0 : kMaxBlocks;
        hipLaunchKernelGGL(wavelet_fwd_fused_kernel<W>, dim3((unsigned)nb), dim3(WF_BLOCK), lds, ctx->stream, x, approx, det, (int)len,
                           (int)levels, rows, b0 * rpb, (int)rpb, (int)bufa);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

template <int W>
int launch_inv_fused(kofft_hip_ctx *ctx, const float *approx, const float *det, const size_t *dl, float *out, size_t n, size_t levels,
                     size_t rows)
{
    static std::atomic<unsigned long long> lds_set{0};
    const size_t total = n << levels;
    size_t rpb = total < kWaveletPackFloats ? kWaveletPackFloats / total : 1;
    if (rpb > rows) rpb = rows;
    const size_t bufh = (rpb * (total / 2) + 3) & ~size_t(3);
    const size_t lds = 2 * bufh * sizeof(float);
    if (lds > (size_t(64) << 10)) {
        const int rc = set_dyn_lds_once(ctx, lds_set, reinterpret_cast<const void *>(wavelet_inv_fused_kernel<W>), lds);
        if (rc) return rc;
    }
    Lens lens{};
    for (size_t l = 0; l < levels; ++l) lens.v[l] = (int)dl[l];
    const size_t blocks = (rows + rpb - 1) / rpb;
    for (size_t b0 = 0; b0 < blocks; b0 += kMaxBlocks) {
        const size_t nb = blocks - b0 < kMaxBlocks ? blocks - b0 : kMaxBlocks;
        hipLaunchKernelGGL(wavelet_inv_fused_kernel<W>, dim3((unsigned)nb), dim3(WF_BLOCK), lds, ctx->stream, approx, det, out, (int)n,
                           (int)levels, rows, b0 * rpb, (int)rpb, (int)bufh, lens);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

// The multi-level route: the fused kernels where tools/bench_wavelet.py measured them faster than level by level on the streaming
// kernels (64 M input floats per call, rows of 1024 .. 16384), per wavelet and direction: a range of row lengths
// (forward: the input, inverse: the output) and of levels.  Outside every range -- rows under 1024 included, where nothing was
// measured -- the calls run level by level.
struct FusedRange {
    size_t min_len, max_len, min_levels, max_levels;
};
constexpr FusedRange kFusedAuto[NFAM][2] = {
    // forward                    inverse
    {{1024, 8192, 2, 64}, {1024, 8192, 2, 5}},    // haar: forward 1.31-1.48x, inverse 1.01-1.25x
    {{1024, 8192, 2, 64}, {8192, 16384, 2, 5}},   // db2: forward 1.02-1.18x, inverse 1.06-1.27x
    {{0, 0, 0, 0}, {8192, 16384, 1, 3}},          // db4: forward never ahead by more than 2 %, inverse 1.16-1.31x
    {{0, 0, 0, 0}, {8192, 16384, 1, 3}},          // sym4: as db4
    {{0, 0, 0, 0}, {8192, 16384, 1, 3}},          // coif1: forward never ahead by more than 4 %, inverse 1.13-1.27x
};

bool use_fused(const kofft_hip_ctx *ctx, int w, bool inverse, size_t len, size_t levels)
{
    if (ctx->wavelet_fused == 0 || len > kWaveletFusedMax) return false;
    if (ctx->wavelet_fused == 2) return true;
    const FusedRange &r = kFusedAuto[w][inverse ? 1 : 0];
    return len >= r.min_len && len <= r.max_len && levels >= r.min_levels && levels <= r.max_levels;
}

}  // namespace

// the coefficient table (8 + 8 floats, +0 past the length; haar: none)
static void wavelet_taps(int w, bool inverse, float *lo, float *hi)
{
    const Taps t = taps(w, inverse);
    for (int k = 0; k < 8; ++k) {
        lo[k] = k < t.len && w != HAAR ? t.lo[k] : 0.0f;
        hi[k] = k < t.len && w != HAAR ? t.hi[k] : 0.0f;
    }
}

// lens[0] = len, lens[l] = ceil(lens[l - 1] / 2); returns sum lens[1..]
static size_t wavelet_lengths(size_t len, size_t levels, size_t *lens)
{
    size_t total = 0;
    lens[0] = len;
    for (size_t l = 1; l <= levels; ++l) {
        lens[l] = (lens[l - 1] + 1) / 2;  // an odd row is padded to lens[l - 1] + 1, then halved
        total += lens[l];
    }
    return total;
}

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched.
static int dwt_check(int w, size_t len, size_t batch, size_t levels, const void *p0, const void *p1, const void *p2, const kofft_hip_ctx *ctx)
{
    if (w < 0 || w >= NFAM) return KOFFT_ERR_INVALID_VALUE;
    if (batch == 0 || len == 0) return KOFFT_OK;
    if (len > kWaveletMaxLen || levels > kWaveletMaxLevels) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !p0 || !p1 || !p2) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int idwt_check(int w, size_t n, size_t batch, size_t levels, const size_t *dl, const void *p0, const void *p1, const void *p2,
               const kofft_hip_ctx *ctx)
{
    if (w < 0 || w >= NFAM) return KOFFT_ERR_INVALID_VALUE;
    if (batch == 0 || n == 0) return KOFFT_OK;
    if (levels > 0 && !dl) return KOFFT_ERR_NULL;  // (the lengths cannot be checked)
    if (levels > kWaveletMaxLevels) return KOFFT_ERR_UNSUPPORTED;  // (before detail_lens[levels - 1] is read)
    bool big = false;
    size_t cur = n;
    for (size_t s = 0; s < levels; ++s) {  // coarsest first, as multi_level_inverse folds them
        const size_t d = dl[levels - 1 - s];
        if (d < cur) return KOFFT_ERR_MISMATCHED_LENGTHS;  // the reference indexes detail[i], i < cur: a panic
        if (d > kWaveletMaxLen) big = true;
        cur = cur > kWaveletMaxLen ? cur : 2 * cur;
    }
    if (big || cur > kWaveletMaxLen || (levels == 0 && n > kWaveletMaxLen)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !p0 || !p1 || !p2) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;
using namespace kofft::wav;

extern "C" {

int kofft_hip_set_wavelet_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::wavelet_fused, on, 0, 2); }

int kofft_hip_wavelet_taps_f32(int wavelet, int inverse, float *lo, float *hi)
{
    if (wavelet < 0 || wavelet > 4) return KOFFT_ERR_INVALID_VALUE;
    if (!lo || !hi) return KOFFT_ERR_NULL;
    wavelet_taps(wavelet, inverse != 0, lo, hi);
    return KOFFT_OK;
}

int kofft_hip_dwt_multi_lengths(size_t len, size_t levels, size_t *lens)
{
    if (levels > kWaveletMaxLevels) return KOFFT_ERR_UNSUPPORTED;
    if (!lens) return KOFFT_ERR_NULL;
    wavelet_lengths(len, levels, lens);
    return KOFFT_OK;
}

int kofft_hip_dwt_f32_dev(kofft_hip_ctx *ctx, int w, const float *d_in, float *d_approx, float *d_detail, size_t len, size_t batch)
{
    int rc = dwt_check(w, len, batch, 0, d_in, d_approx, d_detail, ctx);
    if (rc || batch == 0 || len == 0) return rc;
    const size_t n = len / 2, ob = batch * n * sizeof(float);
    if (any_overlap({{d_in, batch * len * sizeof(float)}, {d_approx, ob}, {d_detail, ob}})) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dispatch(w, [&](auto W) { return launch_fwd<decltype(W)::value>(ctx, d_in, d_approx, d_detail, len, len, batch); });
}

// wavelet::*_forward / *_inverse (one level) on host rows
int kofft_hip_dwt_f32(kofft_hip_ctx *ctx, int w, const float *in, float *approx, float *detail, size_t len, size_t batch)
{
    const int crc = dwt_check(w, len, batch, 0, in, approx, detail, ctx);
    if (crc || batch == 0 || len / 2 == 0) return crc;
    const HostArray<float> a[3] = {{in, nullptr, len}, {nullptr, approx, len / 2}, {nullptr, detail, len / 2}};
    return rows_host_n<float>(ctx, batch, 3, a, nullptr, 0, true, true, [&](float *const *d, const float *, size_t rows) {
        return kofft_hip_dwt_f32_dev(ctx, w, d[0], d[1], d[2], len, rows);
    });
}

int kofft_hip_idwt_f32_dev(kofft_hip_ctx *ctx, int w, const float *d_approx, const float *d_detail, float *d_out, size_t n, size_t batch)
{
    const size_t one = n;
    int rc = idwt_check(w, n, batch, 1, &one, d_approx, d_detail, d_out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    const size_t ib = batch * n * sizeof(float);
    if (any_overlap({{d_approx, ib}, {d_out, 2 * ib}}) || any_overlap({{d_detail, ib}, {d_out, 2 * ib}})) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dispatch(w, [&](auto W) { return launch_inv<decltype(W)::value>(ctx, d_approx, d_detail, d_out, n, n, batch); });
}

int kofft_hip_idwt_f32(kofft_hip_ctx *ctx, int w, const float *approx, const float *detail, float *out, size_t n, size_t batch)
{
    const size_t one = n;
    const int crc = idwt_check(w, n, batch, 1, &one, approx, detail, out, ctx);
    if (crc || batch == 0 || n == 0) return crc;
    const HostArray<float> a[3] = {{approx, nullptr, n}, {detail, nullptr, n}, {nullptr, out, 2 * n}};
    return rows_host_n<float>(ctx, batch, 3, a, nullptr, 0, true, true, [&](float *const *d, const float *, size_t rows) {
        return kofft_hip_idwt_f32_dev(ctx, w, d[0], d[1], d[2], n, rows);
    });
}

int kofft_hip_dwt_multi_f32_dev(kofft_hip_ctx *ctx, int w, const float *d_in, float *d_approx, float *d_details, size_t len, size_t batch,
                                size_t levels)
{
    int rc = dwt_check(w, len, batch, levels, d_in, d_approx, levels ? d_details : d_approx, ctx);
    if (rc || batch == 0 || len == 0) return rc;
    size_t lens[kWaveletMaxLevels + 1];
    const size_t det = wavelet_lengths(len, levels, lens);
    if (any_overlap({{d_in, batch * len * 4}, {d_approx, batch * lens[levels] * 4}, {d_details, batch * det * 4}}))
        return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (levels == 0) {  // the input unchanged, no details
        KOFFT_HIP_TRY(ctx, hipMemcpyAsync(d_approx, d_in, batch * len * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return KOFFT_OK;
    }
    if (use_fused(ctx, w, false, len, levels))
        return dispatch(w, [&](auto W) { return launch_fwd_fused<decltype(W)::value>(ctx, d_in, d_approx, d_details, len, levels, batch); });
    // per level, through two scratch buffers of batch * lens[1] floats
    float *tmp = nullptr;
    if (levels > 1) {
        if ((rc = ensure(ctx, ctx->real_tmp, 2 * batch * lens[1] * sizeof(float)))) return rc;
        tmp = static_cast<float *>(ctx->real_tmp.p);
    }
    const float *src = d_in;
    size_t off = 0;
    for (size_t l = 1; l <= levels; ++l) {
        const size_t c = lens[l - 1];
        float *dst = l == levels ? d_approx : tmp + (l & 1) * batch * lens[1];
        rc = dispatch(w, [&](auto W) { return launch_fwd<decltype(W)::value>(ctx, src, dst, d_details + off, c, c + (c & 1), batch); });
        if (rc) return rc;
        off += batch * lens[l];
        src = dst;
    }
    return KOFFT_OK;
}

// multi_level_forward on host rows (the details are packed level after level, [batch][a_l] each: not row-contiguous, so no pipeline)
int kofft_hip_dwt_multi_f32(kofft_hip_ctx *ctx, int w, const float *in, float *approx, float *details, size_t len, size_t batch, size_t levels)
{
    const int crc = dwt_check(w, len, batch, levels, in, approx, levels ? details : approx, ctx);
    if (crc || batch == 0 || len == 0) return crc;
    size_t lens[kWaveletMaxLevels + 1];
    const size_t det = wavelet_lengths(len, levels, lens);
    const HostArray<float> a[3] = {{in, nullptr, len}, {nullptr, approx, lens[levels]}, {nullptr, details, det}};
    return rows_host_n<float>(ctx, batch, levels ? 3 : 2, a, nullptr, 0, true, false, [&](float *const *d, const float *, size_t rows) {
        return kofft_hip_dwt_multi_f32_dev(ctx, w, d[0], d[1], levels ? d[2] : nullptr, len, rows, levels);
    });
}

int kofft_hip_idwt_multi_f32_dev(kofft_hip_ctx *ctx, int w, const float *d_approx, const float *d_details, const size_t *detail_lens,
                                 float *d_out, size_t n, size_t batch, size_t levels)
{
    int rc = idwt_check(w, n, batch, levels, detail_lens, d_approx, levels ? d_details : d_approx, d_out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    size_t det = 0;
    for (size_t l = 0; l < levels; ++l) det += detail_lens[l];
    const size_t total = n << levels;
    if (any_overlap({{d_approx, batch * n * 4}, {d_out, batch * total * 4}}) || any_overlap({{d_details, batch * det * 4}, {d_out, batch * total * 4}}))
        return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (levels == 0) {
        KOFFT_HIP_TRY(ctx, hipMemcpyAsync(d_out, d_approx, batch * n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return KOFFT_OK;
    }
    if (use_fused(ctx, w, true, total, levels))
        return dispatch(w, [&](auto W) { return launch_inv_fused<decltype(W)::value>(ctx, d_approx, d_details, detail_lens, d_out, n, levels, batch); });
    // per level, coarsest first, through two scratch buffers of batch * total / 2 floats
    float *tmp = nullptr;
    if (levels > 1) {
        if ((rc = ensure(ctx, ctx->real_tmp, batch * total * sizeof(float)))) return rc;
        tmp = static_cast<float *>(ctx->real_tmp.p);
    }
    const float *src = d_approx;
    size_t c = n;
    for (size_t s = 0; s < levels; ++s) {
        const size_t l = levels - 1 - s;
        size_t off = 0;
        for (size_t m = 0; m < l; ++m) off += batch * detail_lens[m];
        float *dst = s == levels - 1 ? d_out : tmp + (s & 1) * batch * (total / 2);
        rc = dispatch(w, [&](auto W) { return launch_inv<decltype(W)::value>(ctx, src, d_details + off, dst, c, detail_lens[l], batch); });
        if (rc) return rc;
        src = dst;
        c *= 2;
    }
    return KOFFT_OK;
}

// multi_level_inverse on host rows
int kofft_hip_idwt_multi_f32(kofft_hip_ctx *ctx, int w, const float *approx, const float *details, const size_t *detail_lens, float *out,
                             size_t n, size_t batch, size_t levels)
{
    const int crc = idwt_check(w, n, batch, levels, detail_lens, approx, levels ? details : approx, out, ctx);
    if (crc || batch == 0 || n == 0) return crc;
    size_t det = 0;
    for (size_t l = 0; l < levels; ++l) det += detail_lens[l];
    const HostArray<float> a[3] = {{approx, nullptr, n}, {nullptr, out, n << levels}, {details, nullptr, det}};
    return rows_host_n<float>(ctx, batch, levels ? 3 : 2, a, nullptr, 0, true, false, [&](float *const *d, const float *, size_t rows) {
        return kofft_hip_idwt_multi_f32_dev(ctx, w, d[0], levels ? d[2] : nullptr, detail_lens, d[1], n, rows, levels);
    });
}

}  // extern "C"
