// k_hilbert_f32.hip -- hilbert::hilbert_analytic (hilbert.rs:13-47) and cepstrum::real_cepstrum (cepstrum.rs:12-33) on float rows:
// every kernel instance of the two families, which share the fused route's body and the composed route's expand kernel
// (fused_rows.hip.h), and their extern "C" entry points.
#include "hilbert_impl.hip.h"
#include "cepstrum_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {
// Argument checks in the reference's order (hilbert.rs:14-19: EmptyInput, then NonPowerOfTwoNoStd), then the complex transform's
// range and the pointers -- all before the context or the device is touched.  The real cepstrum's are the same (cepstrum.rs:13-18).
static int analytic_check(size_t n, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_hilbert_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::hilbert_fused, on); }
int kofft_hip_set_cepstrum_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::cepstrum_fused, on); }

int kofft_hip_hilbert_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const int crc = analytic_check(n, batch, d_in, d_out, ctx);
    if (crc || batch == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (fused_ok(ctx->hilbert_fused, d_in, n))
        return fused_dev<HilbertFused>(ctx, [](auto l) { return hilbert_fused_kernel<decltype(l)::value>; }, d_in, d_out, n, batch);
    return hilbert_composed_dev(ctx, d_in, d_out, n, batch);
}

// on host rows of n reals in, n complex out
int kofft_hip_hilbert_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = analytic_check(n, batch, in, out, ctx);
    if (crc || batch == 0) return crc;
    return rows_host<float>(ctx, in, out, batch, n, 2 * n, nullptr, 0, true, true, [&](float *d_in, float *d_out, const float *, size_t rows) {
        return kofft_hip_hilbert_f32_dev(ctx, d_in, d_out, n, rows);
    });
}

int kofft_hip_cepstrum_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const int crc = analytic_check(n, batch, d_in, d_out, ctx);
    if (crc || batch == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (fused_ok(ctx->cepstrum_fused, d_in, n))
        return fused_dev<CepstrumFused>(ctx, [](auto l) { return cepstrum_fused_kernel<decltype(l)::value>; }, d_in, d_out, n, batch);
    return cepstrum_composed_dev(ctx, d_in, d_out, n, batch);
}

// on host rows of n reals in and out
int kofft_hip_cepstrum_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = analytic_check(n, batch, in, out, ctx);
    if (crc || batch == 0) return crc;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true, [&](float *d_in, float *d_out, const float *, size_t rows) {
        return kofft_hip_cepstrum_f32_dev(ctx, d_in, d_out, n, rows);
    });
}

}  // extern "C"
