// k_planar_f64.hip -- FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on planes of double: every kernel instance of the planar
// layout (planar_impl.hip.h) and its extern "C" entry points.  One translation unit per element type, like the complex transforms, so
// that `make -j` builds them side by side.
#include "planar_impl.hip.h"

using namespace kofft::host;

extern "C" {

int kofft_hip_fft_split_c64(kofft_hip_ctx *ctx, double *re, double *im, size_t n, size_t batch, int inverse)
{
    return planar_host<double>(ctx, re, im, n, batch, inverse);
}
int kofft_hip_dev_fft_split_c64(kofft_hip_ctx *ctx, const double *d_re_in, const double *d_im_in, double *d_re_out, double *d_im_out, size_t n,
                                size_t batch, int inverse)
{
    return planar_dev<double>(ctx, d_re_in, d_im_in, d_re_out, d_im_out, n, batch, inverse);
}

}  // extern "C"
