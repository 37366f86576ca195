// k_real_f32.hip -- real transforms of float rows (rfft.rs:425-508): every kernel instance of the family and its extern "C" entry
// points.
#include "real_impl.hip.h"

using namespace kofft::host;

extern "C" {

int kofft_hip_rfft_f32(kofft_hip_ctx *ctx, const float *in, float *out, const float *window, size_t n, size_t batch)
{
    return rfft_host<float>(ctx, in, out, window, n, batch);
}
int kofft_hip_rfft_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *d_window, size_t n, size_t batch)
{
    return rfft_dev<float>(ctx, d_in, d_out, d_window, n, batch);
}
int kofft_hip_irfft_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    return irfft_host<float>(ctx, in, out, n, batch);
}
int kofft_hip_irfft_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return irfft_dev<float>(ctx, d_in, d_out, n, batch);
}

}  // extern "C"
