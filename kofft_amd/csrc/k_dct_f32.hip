// k_dct_f32.hip -- DctPlanner::plan_dct2 (dct.rs:61-105) on float rows: every kernel instance of the family.
#include "dct_impl.hip.h"

namespace kofft {
namespace host {
// Argument checks in the reference's order where the C ABI can see them: the output length is the caller's (the Python
// planner checks it first, dct.rs:68-70), n = 0 is rfft_direct's EmptyInput (rfft.rs:434), then the inner transform's range.
int dct2_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!complex_len_ok(n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !d_in || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (dct2_fused_ok(ctx, d_in, n)) return dct2_fused_dev(ctx, d_in, d_out, n, batch);
    return dct2_composed_dev(ctx, d_in, d_out, n, batch);
}

}  // namespace host
}  // namespace kofft
