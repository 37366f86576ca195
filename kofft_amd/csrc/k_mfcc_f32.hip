// k_mfcc_f32.hip -- cepstrum::mel_filterbank / mfcc (cepstrum.rs:36-85) on float rows with the filter edges as an input: every
// kernel instance of the family (mfcc_impl.hip.h), the argument checks, the per-context plan cache, the two routes of the MFCC and the
// extern "C" entry points.
#include "mfcc_impl.hip.h"
#include "host_stage.hip.h"

#include <algorithm>

namespace kofft {
namespace host {

constexpr size_t kMfccFusedDefaultMel = 80;     // the measured choice: the fused kernel up to 80 filters (five workgroups per CU) ...
constexpr size_t kMfccFusedDefaultCoeffs = 16;  // ... and 16 coefficients (two passes of its DCT)

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched; mfcc: whether num_coeffs takes part.
static int mel_check(bool mfcc, bool dev, const void *mags, const void *out, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
              size_t num_coeffs, const kofft_hip_ctx *ctx)
{
    if (rows == 0) return KOFFT_OK;
    if (mfcc && num_coeffs > num_mel) return KOFFT_ERR_INVALID_VALUE;  // cepstrum.rs:79
    if (!bins) return KOFFT_ERR_NULL;
    for (size_t i = 0; i < num_mel + 1 && i + 1 != 0; ++i)
        if (bins[i + 1] < bins[i]) return KOFFT_ERR_INVALID_VALUE;  // `bins[m] - bins[m - 1]` underflows in the reference
    if (n_fft > kMelMaxFft || num_mel > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !mags || !out) return KOFFT_ERR_NULL;
    if (dev) {
        const size_t out_row = mfcc ? num_coeffs : num_mel;
        const float *a = static_cast<const float *>(mags), *b = static_cast<const float *>(out);
        if (n_fft && out_row && a < b + rows * out_row && b < a + rows * n_fft) return KOFFT_ERR_INVALID_VALUE;
    }
    return KOFFT_OK;
}

void mel_drop(kofft_hip_ctx *ctx)
{
    for (auto &slot : ctx->mel_slots)
        if (slot.d_plan) (void)hipFree(slot.d_plan);
    ctx->mel_slots.clear();
}

// The device plan of (bins, n_fft, num_mel): a hit moves its slot to the front; a miss builds the plan on the host, uploads it on the
// context's stream (from the slot's own staging vector, which outlives the copy) and, with kMelSlots plans already there, frees the
// least recently used one after a stream synchronisation.
int get_mel_plan(kofft_hip_ctx *ctx, const uint64_t *bins, size_t n_fft, size_t num_mel, const int **out)
{
    auto &slots = ctx->mel_slots;
    for (size_t j = 0; j < slots.size(); ++j) {
        if (slots[j].n_fft == n_fft && slots[j].num_mel == num_mel && std::memcmp(slots[j].bins.data(), bins, (num_mel + 2) * sizeof(uint64_t)) == 0) {
            if (j) std::rotate(slots.begin(), slots.begin() + j, slots.begin() + j + 1);
            *out = static_cast<const int *>(slots[0].d_plan);
            return KOFFT_OK;
        }
    }
    try {
        kofft_mel_slot slot;
        slot.bins.assign(bins, bins + num_mel + 2);
        slot.n_fft = n_fft;
        slot.num_mel = num_mel;
        const size_t ints = kofft_tables::mel_plan_ints(num_mel);
        slot.staged.resize(ints + 2 * n_fft);
        kofft_tables::mel_plan_build(bins, n_fft, num_mel, slot.staged.data(), reinterpret_cast<float *>(slot.staged.data() + ints));
        if (slots.size() >= kMelSlots) {
            KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (slots.back().d_plan) (void)hipFree(slots.back().d_plan);
            slots.pop_back();
        }
        const size_t bytes = slot.staged.size() * sizeof(int);
        if (const char *bad = HipAlloc::alloc(&slot.d_plan, bytes)) return report_failure(ctx, KOFFT_ERR_HIP, "filterbank plan: allocation", bad);
        slots.insert(slots.begin(), std::move(slot));
    } catch (const std::bad_alloc &) {
        return report_failure(ctx, KOFFT_ERR_ALLOC, "filterbank plan", "out of host memory");
    }
    kofft_mel_slot &s = slots.front();
    const hipError_t e = hipMemcpyAsync(s.d_plan, s.staged.data(), s.staged.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s.d_plan);
        slots.erase(slots.begin());
        return report_failure(ctx, KOFFT_ERR_HIP, "filterbank plan: upload", hipGetErrorString(e));
    }
    *out = static_cast<const int *>(s.d_plan);
    return KOFFT_OK;
}

// One launch of mel_kernel over `rows` rows: energies (dct == nullptr) or coefficients
static int launch_mel(kofft_hip_ctx *ctx, const float *d_mags, float *d_out, const int *plan, const float *dct, size_t n_fft, size_t num_mel,
                      size_t nc, size_t rows)
{
    const size_t blocks = (rows + MEL_ROWS - 1) / MEL_ROWS;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    const bool vec = n_fft % 4 == 0 && (reinterpret_cast<size_t>(d_mags) & 15) == 0, fused = dct != nullptr;
    const size_t lds = mel_lds_bytes(fused, num_mel);
    const int ldc = (int)direct_ldc(num_mel);
    auto kern = fused ? (vec ? mel_kernel<true, true> : mel_kernel<false, true>) : (vec ? mel_kernel<true, false> : mel_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(MEL_ROWS), lds, ctx->stream, d_mags, d_out, plan, dct, (int)n_fft, (int)num_mel, (int)nc,
                       ldc, rows);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

int mel_filterbank_dev(kofft_hip_ctx *ctx, const float *d_mags, float *d_energies, size_t n_fft, size_t rows, const uint64_t *bins,
                       size_t num_mel)
{
    int rc = mel_check(false, true, d_mags, d_energies, n_fft, rows, bins, num_mel, 0, ctx);
    if (rc || rows == 0 || num_mel == 0) return rc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int *plan = nullptr;
    rc = get_mel_plan(ctx, bins, n_fft, num_mel, &plan);
    if (rc) return rc;
    return launch_mel(ctx, d_mags, d_energies, plan, nullptr, n_fft, num_mel, 0, rows);
}

// filterbank -> log -> direct DCT-II -> the first num_coeffs columns, through the context's scratch ([energies | dct]: 2 num_mel floats
// per row), scratch_chunk_bytes at a time
static int mfcc_composed_dev(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, const int *plan, size_t n_fft, size_t rows, size_t num_mel,
                             size_t nc)
{
    const size_t row_bytes = 2 * num_mel * sizeof(float);
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, row_bytes, rows);
    int rc = ensure(ctx, ctx->real_tmp, chunk * row_bytes);
    if (rc) return rc;
    float *e = static_cast<float *>(ctx->real_tmp.p), *d = e + chunk * num_mel;
    const unsigned rpb = nc < 256 ? (unsigned)(256 / nc) : 1;
    for (size_t r0 = 0; r0 < rows; r0 += chunk) {
        const size_t nb = rows - r0 < chunk ? rows - r0 : chunk;
        rc = launch_mel(ctx, d_mags + r0 * n_fft, e, plan, nullptr, n_fft, num_mel, 0, nb);
        if (rc) return rc;
        hipLaunchKernelGGL(mel_log_kernel, dim3(flat_blocks(ctx, nb * num_mel, 16)), dim3(256), 0, ctx->stream, e, nb * num_mel);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        rc = direct_dev(ctx, 0, 2, e, d, num_mel, nb);  // dct::dct2 (cepstrum.rs:83)
        if (rc) return rc;
        const size_t groups = (nb + rpb - 1) / rpb;
        const dim3 grid((unsigned)((nc + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));
        hipLaunchKernelGGL(mel_cols_kernel, grid, dim3(256), 0, ctx->stream, d, d_coeffs + r0 * nc, (unsigned)num_mel, (unsigned)nc, nb, rpb);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

// The fused kernel fits up to kMfccFusedMaxMel filters.  It is the default where it measured faster than the composed route by more
// than the spread of the runs at every batch tried: up to 80 filters and up to 16 coefficients, two passes of its DCT
// over the log-mel column -- the 26 .. 80 filters and 12 or 13 coefficients of a speech front end.  Beyond either bound a lane's
// serial DCT and the three or four wavefronts per CU that the log-mel columns leave room for lose to the tiled direct kernel or tie
// with it: 128 x 13 wins by 5 .. 9 % at 4096 and 16384 rows and loses by 25 % at 112500, 80 x 24 ties, 64 x 64 loses by 13 .. 29 %,
// 128 x 128 by a factor of two or more.
static bool mfcc_use_fused(const kofft_hip_ctx *ctx, size_t num_mel, size_t num_coeffs)
{
    if (ctx->mfcc_fused == 0 || num_mel > kMfccFusedMaxMel) return false;
    return ctx->mfcc_fused == 2 || (num_mel <= kMfccFusedDefaultMel && num_coeffs <= kMfccFusedDefaultCoeffs);
}

int mfcc_dev(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
             size_t num_coeffs)
{
    int rc = mel_check(true, true, d_mags, d_coeffs, n_fft, rows, bins, num_mel, num_coeffs, ctx);
    if (rc || rows == 0 || num_mel == 0 || num_coeffs == 0) return rc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int *plan = nullptr;
    rc = get_mel_plan(ctx, bins, n_fft, num_mel, &plan);
    if (rc) return rc;
    if (!mfcc_use_fused(ctx, num_mel, num_coeffs)) return mfcc_composed_dev(ctx, d_mags, d_coeffs, plan, n_fft, rows, num_mel, num_coeffs);
    const float *table = nullptr;
    rc = get_direct_table(ctx, 0, 2, num_mel, &table);  // the cache entry of kofft_hip_dct_direct_f32(ctx, 2, ..) at n = num_mel
    if (rc) return rc;
    return launch_mel(ctx, d_mags, d_coeffs, plan, table, n_fft, num_mel, num_coeffs, rows);
}

// on host rows of n_fft magnitudes in, num_mel energies or num_coeffs coefficients out; the edges stay on the host
static int mel_host(kofft_hip_ctx *ctx, bool mfcc, const float *mags, float *out, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
                    size_t num_coeffs)
{
    const int crc = mel_check(mfcc, false, mags, out, n_fft, rows, bins, num_mel, num_coeffs, ctx);
    if (crc || rows == 0 || num_mel == 0 || (mfcc && num_coeffs == 0)) return crc;
    return rows_host<float>(ctx, mags, out, rows, n_fft, mfcc ? num_coeffs : num_mel, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t nr) {
                                return mfcc ? mfcc_dev(ctx, d_in, d_out, n_fft, nr, bins, num_mel, num_coeffs)
                                            : mel_filterbank_dev(ctx, d_in, d_out, n_fft, nr, bins, num_mel);
                            });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_mfcc_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::mfcc_fused, on, 0, 2); }
int kofft_hip_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *mags, float *energies, size_t n_fft, size_t rows, const uint64_t *bins,
                                 size_t num_mel)
{
    return mel_host(ctx, false, mags, energies, n_fft, rows, bins, num_mel, 0);
}
int kofft_hip_dev_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_energies, size_t n_fft, size_t rows,
                                     const uint64_t *bins, size_t num_mel)
{
    return mel_filterbank_dev(ctx, d_mags, d_energies, n_fft, rows, bins, num_mel);
}
int kofft_hip_mfcc_f32(kofft_hip_ctx *ctx, const float *mags, float *coeffs, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
                       size_t num_coeffs)
{
    return mel_host(ctx, true, mags, coeffs, n_fft, rows, bins, num_mel, num_coeffs);
}
int kofft_hip_dev_mfcc_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const uint64_t *bins,
                           size_t num_mel, size_t num_coeffs)
{
    return mfcc_dev(ctx, d_mags, d_coeffs, n_fft, rows, bins, num_mel, num_coeffs);
}
int kofft_hip_mel_bins_f32(float sample_rate, size_t n_fft, size_t num_filters, uint64_t *bins)
{
    if (num_filters > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!bins) return KOFFT_ERR_NULL;
    kofft_tables::mel_bins_f32(sample_rate, n_fft, num_filters, bins);
    return KOFFT_OK;
}

}  // extern "C"
