// k_real_f64.hip -- real transforms of double rows (rfft.rs:425-508): every kernel instance of the family and its extern "C" entry
// points.
#include "real_impl.hip.h"

using namespace kofft::host;

extern "C" {

int kofft_hip_rfft_f64(kofft_hip_ctx *ctx, const double *in, double *out, const double *window, size_t n, size_t batch)
{
    return rfft_host<double>(ctx, in, out, window, n, batch);
}
int kofft_hip_rfft_f64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, const double *d_window, size_t n, size_t batch)
{
    return rfft_dev<double>(ctx, d_in, d_out, d_window, n, batch);
}
int kofft_hip_irfft_f64(kofft_hip_ctx *ctx, const double *in, double *out, size_t n, size_t batch)
{
    return irfft_host<double>(ctx, in, out, n, batch);
}
int kofft_hip_irfft_f64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch)
{
    return irfft_dev<double>(ctx, d_in, d_out, n, batch);
}

}  // extern "C"
