// k_complex_f64.hip -- Complex<double> transforms (fft.rs:1054-1174): the single-pass kernels (one workgroup per transform, the CU's
// register file), the Radix4 arm and the extern "C" entry points of both.  The factor path lives in k_big_f64.hip and the Bluestein arm in k_blue_f64.hip: three translation
// units per element type so that `make -j` builds them side by side (round 6: one unit took 70 s of a 90 s build).
#include "complex_impl.hip.h"

namespace kofft {
namespace host {
extern template int fft_big_dev<double, false>(kofft_hip_ctx *, const double *, double *, size_t, size_t);       // k_big_f64.hip
extern template int fft_big_dev<double, true>(kofft_hip_ctx *, const double *, double *, size_t, size_t);
extern template int fft_bluestein_dev<double, false>(kofft_hip_ctx *, const double *, double *, size_t, size_t);  // k_blue_f64.hip
extern template int fft_bluestein_dev<double, true>(kofft_hip_ctx *, const double *, double *, size_t, size_t);
template int fft_dev<double>(kofft_hip_ctx *, const double *, double *, size_t, size_t, int);
}  // namespace host
}  // namespace kofft

using namespace kofft::host;

extern "C" {

int kofft_hip_fft_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch, int inverse) { return fft_host<double>(ctx, data, n, batch, inverse); }
int kofft_hip_fft_c64_dev(kofft_hip_ctx *ctx, double *d_data, size_t n, size_t batch, int inverse)
{
    return fft_dev<double>(ctx, d_data, d_data, n, batch, inverse);
}
int kofft_hip_fft_c64_dev_oop(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch, int inverse)
{
    return fft_dev<double>(ctx, d_in, d_out, n, batch, inverse);
}
int kofft_hip_fft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch) { return fft_radix4_host<double>(ctx, data, n, batch, 0); }
int kofft_hip_ifft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch) { return fft_radix4_host<double>(ctx, data, n, batch, 1); }
int kofft_hip_fft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<double>(ctx, d_in, d_out, n, batch, 0);
}
int kofft_hip_ifft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<double>(ctx, d_in, d_out, n, batch, 1);
}
int kofft_hip_fft_c64_strided(kofft_hip_ctx *ctx, double *data, size_t data_len, size_t stride, size_t n, int inverse)
{
    return fft_strided_host<double>(ctx, data, data_len, stride, n, inverse);
}

}  // extern "C"
