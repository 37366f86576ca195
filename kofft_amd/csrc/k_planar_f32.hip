// k_planar_f32.hip -- FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on planes of float: every kernel instance of the planar
// layout (planar_impl.hip.h) and its extern "C" entry points.  One translation unit per element type, like the complex transforms, so
// that `make -j` builds them side by side.
#include "planar_impl.hip.h"

using namespace kofft::host;

extern "C" {

int kofft_hip_set_split_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::planar_fused, on); }
int kofft_hip_fft_split_c32(kofft_hip_ctx *ctx, float *re, float *im, size_t n, size_t batch, int inverse)
{
    return planar_host<float>(ctx, re, im, n, batch, inverse);
}
int kofft_hip_dev_fft_split_c32(kofft_hip_ctx *ctx, const float *d_re_in, const float *d_im_in, float *d_re_out, float *d_im_out, size_t n,
                                size_t batch, int inverse)
{
    return planar_dev<float>(ctx, d_re_in, d_im_in, d_re_out, d_im_out, n, batch, inverse);
}

}  // extern "C"
