// k_dct_f32.hip -- DctPlanner::plan_dct2 (dct.rs:61-105) on float rows: every kernel instance of the family and its
// extern "C" entry points.
#include "dct_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {
// Argument checks in the reference's order where the C ABI can see them: the output length is the caller's (the Python
// planner checks it first, dct.rs:68-70), n = 0 is rfft_direct's EmptyInput (rfft.rs:434), then the inner transform's range.
static int dct2_check(size_t n, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!complex_len_ok(n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_dct_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::dct_fused, on); }

int kofft_hip_dct2_table_f32(size_t n, float *cs)
{
    if (!cs && n) return KOFFT_ERR_NULL;
    kofft_tables::dct2_table_f32(n, cs);
    return KOFFT_OK;
}

int kofft_hip_dct2_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const int crc = dct2_check(n, batch, d_in, d_out, ctx);
    if (crc || batch == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (dct2_fused_ok(ctx, d_in, n)) return dct2_fused_dev(ctx, d_in, d_out, n, batch);
    return dct2_composed_dev(ctx, d_in, d_out, n, batch);
}

// on host rows of n reals in and out
int kofft_hip_dct2_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = dct2_check(n, batch, in, out, ctx);
    if (crc || batch == 0) return crc;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true, [&](float *d_in, float *d_out, const float *, size_t rows) {
        return kofft_hip_dct2_f32_dev(ctx, d_in, d_out, n, rows);
    });
}

}  // extern "C"
