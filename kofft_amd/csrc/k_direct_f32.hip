// k_direct_f32.hip -- dct::dct1..dct4 (dct.rs:108-176) and dst::dst1..dst4 (dst.rs:89-146) on float rows: every kernel instance of
// the family (direct_impl.hip.h) and its extern "C" entry points.
#include "direct_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {
// Checks in the order of include/kofft_hip.h, all before the context or the device is touched: the type, batch == 0, n == 0 (the
// reference returns an empty result, except DCT-III / DST-III, which index input[0] unchecked: EMPTY_INPUT here), the table bound,
// then the pointers.
static int direct_check(int family, int type, size_t n, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    (void)family;
    if (type < 1 || type > 4) return KOFFT_ERR_INVALID_VALUE;
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return type == 3 ? KOFFT_ERR_EMPTY_INPUT : KOFFT_OK;
    if (n > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

int direct_dev(kofft_hip_ctx *ctx, int family, int type, const float *d_in, float *d_out, size_t n, size_t batch)
{
    int rc = direct_check(family, type, n, batch, d_in, d_out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    // tiles of one row run in different workgroups: an output that overlaps the input would be read after it is written
    if (d_in < d_out + batch * n && d_out < d_in + batch * n) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const float *table = nullptr;
    rc = get_direct_table(ctx, family, type, n, &table);
    if (rc) return rc;
    size_t ib, ie;
    kofft_tables::direct_range(family, type, n, &ib, &ie);
    if (family == 0 && type == 1) return launch_direct<DIR_DCT1>(ctx, d_in, d_out, table, n, n, batch, ib, ie);
    if (type == 3) return launch_direct<DIR_HALF>(ctx, d_in, d_out, table, n, n, batch, ib, ie);
    return launch_direct<DIR_ZERO>(ctx, d_in, d_out, table, n, n, batch, ib, ie);
}

int direct_zero_sums(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *table, size_t n, size_t nk, size_t batch)
{
    return launch_direct<DIR_ZERO>(ctx, d_in, d_out, table, n, nk, batch, 0, n);
}

// on host rows of n reals in and out
static int direct_host(kofft_hip_ctx *ctx, int family, int type, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = direct_check(family, type, n, batch, in, out, ctx);
    if (crc || batch == 0 || n == 0) return crc;
    // No pipeline: the whole input is on the device before any output is written back, so in == out works (the reference's
    // batch_* are in place).
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, false,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return direct_dev(ctx, family, type, d_in, d_out, n, rows); });
}

static int direct_table(int family, int type, size_t n, float *c)
{
    if (type < 1 || type > 4) return KOFFT_ERR_INVALID_VALUE;
    if (n == 0) return KOFFT_OK;
    if (n > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!c) return KOFFT_ERR_NULL;
    kofft_tables::direct_table_f32(family, type, n, n, c);
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_direct_tiled(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::direct_tiled, on); }
int kofft_hip_dct_direct_table_f32(int type, size_t n, float *c) { return direct_table(0, type, n, c); }
int kofft_hip_dst_direct_table_f32(int type, size_t n, float *c) { return direct_table(1, type, n, c); }
int kofft_hip_dst_planner_table_f32(int type, size_t n, float *out)
{
    if (type < 2 || type > 4) return KOFFT_ERR_INVALID_VALUE;
    if (n == 0) return KOFFT_OK;
    if (!out) return KOFFT_ERR_NULL;
    kofft_tables::dst_planner_f32(type, n, out);
    return KOFFT_OK;
}
int kofft_hip_dst_planner_table_f64(int type, size_t n, double *out)
{
    if (type < 2 || type > 4) return KOFFT_ERR_INVALID_VALUE;
    if (n == 0) return KOFFT_OK;
    if (!out) return KOFFT_ERR_NULL;
    kofft_tables::dst_planner_f64(type, n, out);
    return KOFFT_OK;
}
int kofft_hip_dct_direct_f32(kofft_hip_ctx *ctx, int type, const float *in, float *out, size_t n, size_t batch)
{
    return direct_host(ctx, 0, type, in, out, n, batch);
}
int kofft_hip_dct_direct_f32_dev(kofft_hip_ctx *ctx, int type, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return direct_dev(ctx, 0, type, d_in, d_out, n, batch);
}
int kofft_hip_dst_direct_f32(kofft_hip_ctx *ctx, int type, const float *in, float *out, size_t n, size_t batch)
{
    return direct_host(ctx, 1, type, in, out, n, batch);
}
int kofft_hip_dst_direct_f32_dev(kofft_hip_ctx *ctx, int type, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return direct_dev(ctx, 1, type, d_in, d_out, n, batch);
}

}  // extern "C"
