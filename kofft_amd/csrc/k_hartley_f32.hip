// k_hartley_f32.hip -- hartley::dht (hartley.rs:12-57) on float rows: the table kernel (hartley_impl.hip.h), the table cache and the
// hand-over to the kernels of the direct DCT / DST, and the extern "C" entry points.
#include "hartley_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

// Checks in the order of include/kofft_hip.h, all before the context or the device is touched.
static int dht_check(size_t n, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_OK;  // hartley.rs:13-14: an empty result
    if (n > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

// The n x direct_ldc(n) table, built at the first call of a (context, n) and kept until the context is destroyed: on the device by
// dht_table_kernel (stream-ordered before the sums that read it; a later kofft_hip_set_stream orders the new stream after it), or
// on the host and uploaded (kofft_hip_set_dht_table_device(ctx, 0)).
static int get_dht_table(kofft_hip_ctx *ctx, size_t n, const float **out)
{
    const size_t ldc = direct_ldc(n), bytes = n * ldc * sizeof(float);
    const bool on_device = ctx->dht_table_device;
    return device_table(ctx, kTableDht, n, bytes, on_device ? "dht table launch" : "dht table upload", out, [&](void *d, std::string &why) {
        if (!on_device) {
            std::vector<float> host(n * ldc);
            kofft_tables::dht_table_f32(n, ldc, host.data());
            return upload_table(d, host.data(), bytes, why);
        }
        const float factor = (2.0f * 3.14159265358979323846f) / (float)n;  // hartley.rs:15
        const dim3 grid((unsigned)((ldc + 4 * DHT_BLOCK - 1) / (4 * DHT_BLOCK)), (unsigned)n);
        hipLaunchKernelGGL(dht_table_kernel, grid, dim3(DHT_BLOCK), 0, ctx->stream, static_cast<float *>(d), (int)n, (int)ldc, factor);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) why = hipGetErrorString(e);
        return e == hipSuccess ? KOFFT_OK : KOFFT_ERR_HIP;
    });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_dht_table_device(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::dht_table_device, on); }

int kofft_hip_dht_table_f32(size_t n, float *H)
{
    if (n == 0) return KOFFT_OK;
    if (n > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!H) return KOFFT_ERR_NULL;
    kofft_tables::dht_table_f32(n, n, H);
    return KOFFT_OK;
}

int kofft_hip_dev_dht_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    int rc = dht_check(n, batch, d_in, d_out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    // tiles of one row run in different workgroups: an output that overlaps the input would be read after it is written
    if (d_in < d_out + batch * n && d_out < d_in + batch * n) return KOFFT_ERR_INVALID_VALUE;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const float *table = nullptr;
    rc = get_dht_table(ctx, n, &table);
    if (rc) return rc;
    return direct_zero_sums(ctx, d_in, d_out, table, n, n, batch);
}

// on host rows of n reals in and out
int kofft_hip_dht_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = dht_check(n, batch, in, out, ctx);
    if (crc || batch == 0 || n == 0) return crc;
    // No pipeline, like the direct sums: in == out works (hartley::batch is in place).
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, false,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return kofft_hip_dev_dht_f32(ctx, d_in, d_out, n, rows); });
}

}  // extern "C"
