// k_cepstrum_f32.hip -- cepstrum::real_cepstrum (cepstrum.rs:12-33) on float rows: every kernel instance of the family, in the
// translation unit of the Hilbert family.  cepstrum_impl.hip.h reuses hilbert_impl.hip.h (its geometry, forward transform and
// expand kernel), and that header defines plain kernels (hilbert_expand_kernel, hilbert_mask_kernel): a second translation unit
// that includes it defines their host-side symbols a second time, and the library does not link.  So this file takes
// k_hilbert_f32.hip in as it stands, and the Makefile builds this object in the place of k_hilbert_f32.o.
#include "k_hilbert_f32.hip"
#include "cepstrum_impl.hip.h"

namespace kofft {
namespace host {
// Argument checks in the reference's order (cepstrum.rs:13-18: EmptyInput, then NonPowerOfTwoNoStd), then the complex transform's
// range and the pointers -- all before the context or the device is touched.
int cepstrum_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !d_in || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (cepstrum_fused_ok(ctx, d_in, n)) return cepstrum_fused_dev(ctx, d_in, d_out, n, batch);
    return cepstrum_composed_dev(ctx, d_in, d_out, n, batch);
}

}  // namespace host
}  // namespace kofft
