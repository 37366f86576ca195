// k_complex_f32.hip -- Complex<float> transforms (fft.rs:1054-1174): the single-pass kernels (one workgroup per transform, the CU's
// register file), the Radix4 arm and the extern "C" entry points of both.  The factor path lives in k_big_f32.hip and the Bluestein arm in k_blue_f32.hip: three translation
// units per element type so that `make -j` builds them side by side (round 6: one unit took 70 s of a 90 s build).
#include "complex_impl.hip.h"

namespace kofft {
namespace host {
extern template int fft_big_dev<float, false>(kofft_hip_ctx *, const float *, float *, size_t, size_t);       // k_big_f32.hip
extern template int fft_big_dev<float, true>(kofft_hip_ctx *, const float *, float *, size_t, size_t);
extern template int fft_bluestein_dev<float, false>(kofft_hip_ctx *, const float *, float *, size_t, size_t);  // k_blue_f32.hip
extern template int fft_bluestein_dev<float, true>(kofft_hip_ctx *, const float *, float *, size_t, size_t);
template int fft_dev<float>(kofft_hip_ctx *, const float *, float *, size_t, size_t, int);
}  // namespace host
}  // namespace kofft

using namespace kofft::host;

extern "C" {

int kofft_hip_fft_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch, int inverse) { return fft_host<float>(ctx, data, n, batch, inverse); }
int kofft_hip_fft_c32_dev(kofft_hip_ctx *ctx, float *d_data, size_t n, size_t batch, int inverse)
{
    return fft_dev<float>(ctx, d_data, d_data, n, batch, inverse);
}
int kofft_hip_fft_c32_dev_oop(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch, int inverse)
{
    return fft_dev<float>(ctx, d_in, d_out, n, batch, inverse);
}
int kofft_hip_fft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch) { return fft_radix4_host<float>(ctx, data, n, batch, 0); }
int kofft_hip_ifft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch) { return fft_radix4_host<float>(ctx, data, n, batch, 1); }
int kofft_hip_fft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<float>(ctx, d_in, d_out, n, batch, 0);
}
int kofft_hip_ifft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<float>(ctx, d_in, d_out, n, batch, 1);
}
int kofft_hip_fft_c32_strided(kofft_hip_ctx *ctx, float *data, size_t data_len, size_t stride, size_t n, int inverse)
{
    return fft_strided_host<float>(ctx, data, data_len, stride, n, inverse);
}

}  // extern "C"
