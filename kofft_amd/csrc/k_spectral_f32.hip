// k_spectral_f32.hip -- czt::czt_f32 (czt.rs:16-54) and goertzel::goertzel_f32 (goertzel.rs:16-36) on float rows: every kernel
// instance of the family (spectral_impl.hip.h), the table cache, the route and the extern "C" entry points.
#include "spectral_impl.hip.h"
#include "host_stage.hip.h"

#include <algorithm>

namespace kofft {
namespace host {

constexpr size_t kCztMax = 4096;  // the longest row and the most bins: the table is 128 MiB there
constexpr size_t kGoertzelMaxLen = size_t(1) << 26;
constexpr size_t kGoertzelMaxFreqs = 1024;

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched.
static int czt_check(size_t n, size_t m, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    if (batch == 0 || m == 0) return KOFFT_OK;
    if (n > kCztMax || m > kCztMax) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !out || (!in && n != 0)) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int goertzel_check(size_t n, size_t batch, float sample_rate, const void *freqs, size_t nfreq, const void *in, const void *out,
                   const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;                // goertzel.rs:17-19
    if (sample_rate <= 0.0f) return KOFFT_ERR_INVALID_VALUE;  // goertzel.rs:20-22 (a NaN rate passes, as there)
    if (nfreq == 0) return KOFFT_OK;
    if (n > kGoertzelMaxLen || nfreq > kGoertzelMaxFreqs) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out || !freqs) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static void free_slot(kofft_spectral_slot &s)
{
    if (s.d_small) (void)hipFree(s.d_small);
    if (s.d_table) (void)hipFree(s.d_table);
    s.d_small = s.d_table = nullptr;
}

void spectral_drop(kofft_hip_ctx *ctx)
{
    for (auto &s : ctx->czt_slots) free_slot(s);
    ctx->czt_slots.clear();
    if (ctx->goertzel_coeff) (void)hipFree(ctx->goertzel_coeff);
    ctx->goertzel_coeff = nullptr;
    ctx->goertzel_last.clear();
}

// The slot of `key` at the front of `list`: found (moved there), or new with `small` (count floats) uploaded; a full list first loses
// its least recently used slot, freed once the stream has run dry (work in flight may still read it).
static int get_slot(kofft_hip_ctx *ctx, std::vector<kofft_spectral_slot> &list, const std::vector<unsigned> &key, const float *small,
                    size_t count, kofft_spectral_slot **out)
{
    for (size_t j = 0; j < list.size(); ++j) {
        if (list[j].key == key) {
            if (j) std::rotate(list.begin(), list.begin() + j, list.begin() + j + 1);
            *out = &list[0];
            return KOFFT_OK;
        }
    }
    if (list.size() >= kSpectralSlots) {
        KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        free_slot(list.back());
        list.pop_back();
    }
    void *d = nullptr;
    KOFFT_HIP_TRY(ctx, hipMalloc(&d, count * sizeof(float)));
    // synchronous copy: once per slot
    const hipError_t e = hipMemcpy(d, small, count * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        ctx->last_error = std::string("spectral table upload: ") + hipGetErrorString(e);
        return KOFFT_ERR_HIP;
    }
    kofft_spectral_slot s;
    s.key = key;
    s.d_small = d;
    list.insert(list.begin(), std::move(s));
    *out = &list[0];
    return KOFFT_OK;
}

static unsigned f32_bits(float v)
{
    unsigned u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// From which batch a table pays (route 0).  Per (row, bin, sample) the SUM mode spends the recurrence and the term (10 multiplies
// and adds) besides the sum itself (4), the table route the sum alone on the tiled kernel's packed arithmetic -- but a fresh table costs
// one walk of all n samples by only ldc / 2 lanes and n * ldc * 4 bytes written and read back.  From that count: a cached table from
// batch 2, a fresh one from batch 8.  Not measured yet: tools/bench_spectral.py sum prints the timings to set it from.
inline bool czt_use_table(size_t n, size_t m, size_t batch, bool cached)
{
    (void)n;
    (void)m;
    return batch >= (cached ? 2u : 8u);
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_czt_route(kofft_hip_ctx *ctx, int mode) { return set_route(ctx, &kofft_hip_ctx::czt_route, mode, 0, 2); }

int kofft_hip_czt_table_f32(size_t n, size_t m, float wr, float wi, float ar, float ai, float *C)
{
    if (n == 0 || m == 0) return KOFFT_OK;
    if (n > kCztMax || m > kCztMax) return KOFFT_ERR_UNSUPPORTED;
    if (!C) return KOFFT_ERR_NULL;
    kofft_tables::czt_table_f32(n, m, wr, wi, ar, ai, 2 * m, C);
    return KOFFT_OK;
}

int kofft_hip_goertzel_coeff_f32(size_t n, float sample_rate, const float *target_freqs, size_t nfreq, float *coeff)
{
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (sample_rate <= 0.0f) return KOFFT_ERR_INVALID_VALUE;
    if (nfreq == 0) return KOFFT_OK;
    if (n > kGoertzelMaxLen || nfreq > kGoertzelMaxFreqs) return KOFFT_ERR_UNSUPPORTED;
    if (!target_freqs || !coeff) return KOFFT_ERR_NULL;
    kofft_tables::goertzel_coeff_f32(n, sample_rate, target_freqs, nfreq, coeff);
    return KOFFT_OK;
}

int kofft_hip_dev_czt_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t m, float wr, float wi, float ar, float ai,
                          size_t batch)
{
    int rc = czt_check(n, m, batch, d_in, d_out, ctx);
    if (rc || batch == 0 || m == 0) return rc;
    // the tiles of one row run in different workgroups: an output that overlaps the input would be read after it is written
    if (n && d_in < d_out + batch * 2 * m && d_out < d_in + batch * n) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) {  // the loop body never runs: m bins of (+0, +0) per row
        KOFFT_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, batch * 2 * m * sizeof(float), ctx->stream));
        return KOFFT_OK;
    }
    const std::vector<unsigned> key = {(unsigned)n, (unsigned)m, f32_bits(wr), f32_bits(wi), f32_bits(ar), f32_bits(ai)};
    kofft_spectral_slot *slot = nullptr;
    {
        bool have = false;
        for (const auto &s : ctx->czt_slots) have = have || s.key == key;
        std::vector<float> pows;
        if (!have) {
            try {
                pows.resize(2 * m + 2 * n);
            } catch (const std::bad_alloc &) {
                return KOFFT_ERR_ALLOC;
            }
            kofft_tables::czt_wpow_f32(m, wr, wi, pows.data());
            kofft_tables::czt_apow_f32(n, ar, ai, pows.data() + 2 * m);
        }
        rc = get_slot(ctx, ctx->czt_slots, key, pows.data(), 2 * m + 2 * n, &slot);
        if (rc) return rc;
    }
    const float *d_wpow = static_cast<const float *>(slot->d_small), *d_apow = d_wpow + 2 * m;
    const bool table = ctx->czt_route == 2 || (ctx->czt_route == 0 && czt_use_table(n, m, batch, slot->d_table != nullptr));
    if (!table) {
        const int rpb = m < 256 ? (int)(256 / m) : 1;
        const size_t groups = (batch + rpb - 1) / rpb;
        const dim3 grid((unsigned)((m + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));
        hipLaunchKernelGGL(czt_recur_kernel<CZT_SUM>, grid, dim3(256), 0, ctx->stream, d_in, d_wpow, d_apow, d_out, (int)n, (int)m, (int)m, 0,
                           batch, rpb);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return KOFFT_OK;
    }
    const size_t ldc = direct_ldc(2 * m);
    if (!slot->d_table) {
        KOFFT_HIP_TRY(ctx, hipMalloc(&slot->d_table, n * ldc * sizeof(float)));
        // one wavefront per workgroup: the ldc / 2 lanes (a multiple of 64) spread over as many CUs as they can
        hipLaunchKernelGGL(czt_recur_kernel<CZT_TABLE>, dim3((unsigned)(ldc / 2 / 64)), dim3(64), 0, ctx->stream, nullptr, d_wpow, d_apow,
                           static_cast<float *>(slot->d_table), (int)n, (int)(ldc / 2), (int)m, (int)ldc, size_t(1), 1);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return direct_zero_sums(ctx, d_in, d_out, static_cast<const float *>(slot->d_table), n, 2 * m, batch);
}

// on host rows: n reals in, m complex out
int kofft_hip_czt_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t m, float wr, float wi, float ar, float ai, size_t batch)
{
    const int crc = czt_check(n, m, batch, in, out, ctx);
    if (crc || batch == 0 || m == 0) return crc;
    if (n == 0) {  // the loop body never runs: (+0, +0) in every bin
        std::memset(out, 0, batch * 2 * m * sizeof(float));
        return KOFFT_OK;
    }
    return rows_host<float>(ctx, in, out, batch, n, 2 * m, nullptr, 0, true, false, [&](float *d_in, float *d_out, const float *, size_t rows) {
        return kofft_hip_dev_czt_f32(ctx, d_in, d_out, n, m, wr, wi, ar, ai, rows);
    });
}

static int goertzel_launch(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *d_coeff, size_t n, size_t batch, size_t nfreq)
{
    const int fpb = nfreq < 256 ? (int)nfreq : 256, rpb = 256 / fpb;
    const size_t groups = (batch + rpb - 1) / rpb;
    const bool vec_in = (n % 4) == 0 && (reinterpret_cast<size_t>(d_in) & 15) == 0;
    const dim3 grid((unsigned)((nfreq + fpb - 1) / fpb), (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(goertzel_kernel, grid, dim3(256), 0, ctx->stream, d_in, d_coeff, d_out, (int)n, (int)nfreq, batch, fpb, rpb, groups,
                       vec_in);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

int kofft_hip_dev_goertzel_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch, float sample_rate,
                               const float *target_freqs, size_t nfreq)
{
    int rc = goertzel_check(n, batch, sample_rate, target_freqs, nfreq, d_in, d_out, ctx);
    if (rc || batch == 0 || nfreq == 0) return rc;
    // a workgroup writes its rows' outputs while others still read their rows
    if (d_in < d_out + batch * nfreq && d_out < d_in + batch * n) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<float> coeff(nfreq);
    kofft_tables::goertzel_coeff_f32(n, sample_rate, target_freqs, nfreq, coeff.data());
    // One buffer of kGoertzelMaxFreqs floats per context.  The coefficients go over in kernel arguments, stream-ordered after the
    // kernels that still read the previous set; a call with the bits of the last set uploads nothing.
    if (!ctx->goertzel_coeff) KOFFT_HIP_TRY(ctx, hipMalloc(&ctx->goertzel_coeff, kGoertzelMaxFreqs * sizeof(float)));
    float *d_coeff = static_cast<float *>(ctx->goertzel_coeff);
    if (ctx->goertzel_last.size() != nfreq || std::memcmp(ctx->goertzel_last.data(), coeff.data(), nfreq * sizeof(float)) != 0) {
        ctx->goertzel_last.clear();  // (a failed launch below leaves the buffer undefined)
        for (size_t j0 = 0; j0 < nfreq; j0 += SP_FILL) {
            sp_fill_chunk c;
            const size_t cnt = nfreq - j0 < (size_t)SP_FILL ? nfreq - j0 : (size_t)SP_FILL;
            std::memcpy(c.v, coeff.data() + j0, cnt * sizeof(float));
            std::memset(c.v + cnt, 0, (SP_FILL - cnt) * sizeof(float));
            hipLaunchKernelGGL(spectral_fill_kernel, dim3(1), dim3(SP_FILL), 0, ctx->stream, d_coeff + j0, c, (int)cnt);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        ctx->goertzel_last = coeff;
    }
    return goertzel_launch(ctx, d_in, d_out, d_coeff, n, batch, nfreq);
}

// on host rows against nfreq frequencies: the coefficients go up as the side input
int kofft_hip_goertzel_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch, float sample_rate,
                           const float *target_freqs, size_t nfreq)
{
    const int crc = goertzel_check(n, batch, sample_rate, target_freqs, nfreq, in, out, ctx);
    if (crc || batch == 0 || nfreq == 0) return crc;
    std::vector<float> coeff(nfreq);
    kofft_tables::goertzel_coeff_f32(n, sample_rate, target_freqs, nfreq, coeff.data());
    return rows_host<float>(ctx, in, out, batch, n, nfreq, coeff.data(), nfreq, true, true,
                            [&](float *d_in, float *d_out, const float *d_coeff, size_t rows) { return goertzel_launch(ctx, d_in, d_out, d_coeff, n, rows, nfreq); });
}

}  // extern "C"
