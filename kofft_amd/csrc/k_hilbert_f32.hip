// k_hilbert_f32.hip -- hilbert::hilbert_analytic (hilbert.rs:13-47) and cepstrum::real_cepstrum (cepstrum.rs:12-33) on float rows:
// every kernel instance of the two families, which share the fused route's body and the composed route's expand kernel
// (fused_rows.hip.h).
#include "hilbert_impl.hip.h"
#include "cepstrum_impl.hip.h"

namespace kofft {
namespace host {
// Argument checks in the reference's order (hilbert.rs:14-19: EmptyInput, then NonPowerOfTwoNoStd), then the complex transform's
// range and the pointers -- all before the context or the device is touched.
int hilbert_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !d_in || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (fused_ok(ctx->hilbert_fused, d_in, n))
        return fused_dev<HilbertFused>(ctx, [](auto l) { return hilbert_fused_kernel<decltype(l)::value>; }, d_in, d_out, n, batch);
    return hilbert_composed_dev(ctx, d_in, d_out, n, batch);
}

// Argument checks in the reference's order (cepstrum.rs:13-18: EmptyInput, then NonPowerOfTwoNoStd), as hilbert_dev.
int cepstrum_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !d_in || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (fused_ok(ctx->cepstrum_fused, d_in, n))
        return fused_dev<CepstrumFused>(ctx, [](auto l) { return cepstrum_fused_kernel<decltype(l)::value>; }, d_in, d_out, n, batch);
    return cepstrum_composed_dev(ctx, d_in, d_out, n, batch);
}

}  // namespace host
}  // namespace kofft
