// k_stft_onesided.hip -- the one-sided STFT over rows of signals and its inverse on device and host pointers, with their
// extern "C" entry points.  Forward: the frames of k_stft_rows.hip's full STFT with bins 0 .. n/2 of every frame kept, dense rows of K = n/2 + 1 complex values, bit for bit
// the prefix of the full frames (StftRowsOf<StftHalfIO>: the same kernels, the same arithmetic, fewer stores).  Inverse:
// stft::inverse_parallel (stft.rs:289-343) of the Hermitian completion of such frames.
#include "host_common.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

// the completed frame F[k] = H[k] for k < bins, (H[n - k].re, -H[n - k].im) above; the imaginary parts of H[0] and H[n/2] as given.
// One bin of F per thread; `half` is only read.
__global__ __launch_bounds__(256) void expand_half_kernel(const cpx<float> *__restrict__ half, cpx<float> *__restrict__ full,
                                                          const size_t win_len, const size_t bins, const size_t total /* transforms * win_len */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t t = idx / win_len, k = idx - t * win_len;
    const cpx<float> *h = half + t * bins;
    if (k < bins) {
        full[idx] = h[k];
    } else {
        const cpx<float> c = h[win_len - k];
        full[idx] = mk<float>(c.re, -c.im);
    }
}

int expand_half(kofft_hip_ctx *ctx, const float *d_half, float *d_full, size_t nt, size_t win_len)
{
    const size_t total = nt * win_len;
    if (total == 0) return KOFFT_OK;
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(expand_half_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const cpx<float> *>(d_half),
                       reinterpret_cast<cpx<float> *>(d_full), win_len, win_len / 2 + 1, total);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// stft_rows_check's checks in its order, then the size of the one-sided output
static int stft_onesided_check(bool host_form, size_t rows, size_t len, size_t row_stride, size_t win_len, size_t hop, size_t frames)
{
    const int crc = stft_rows_check(host_form, false, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    const size_t total = rows * frames, bins = win_len / 2 + 1;  // (rows * frames * win_len passed the check above)
    if (bins > (SIZE_MAX >> 4) / total) return KOFFT_ERR_UNSUPPORTED;
    return KOFFT_OK;
}

// frames [f0, f0 + nf) of each of nrows rows (f0 != 0: one row), dense at d_out: the one-sided STFT's kernels on a rectangle of the
// batch, for the chunk walks that keep the frames in the context's scratch (framed_produce; k_welch_f32.hip)
int stft_onesided_piece(kofft_hip_ctx *ctx, const float *d_signal, size_t nrows, size_t len, size_t row_stride, const float *d_window,
                        size_t win_len, size_t hop, size_t f0, size_t nf, float *d_out)
{
    StftHalfRowsIO io{};
    fill_rows_io(io, d_signal, nrows, len, row_stride, d_window, win_len, hop, nf);
    io.start0 = (f0 && hop > len / f0) ? len : f0 * hop;  // (a start at or past len: silence, as every frame after it; mags_piece's form)
    io.out = reinterpret_cast<cpx<float> *>(d_out);
    return dispatch<float, EPI_STORE>(ctx, io, win_len, nrows * nf);
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dev_stft_onesided_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                    const float *d_window, size_t win_len, size_t hop, float *d_out, size_t frames)
{
    const int crc = stft_onesided_check(false, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (!ctx || (!d_signal && len) || !d_window || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = rows * frames, bins = win_len / 2 + 1;
    FramedSrc s;
    (void)framed_src(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, &s);  // (the caller's window: nothing to fail)
    if (!s.kernels) {
        // any other window length: the composed frames in the context's scratch, at most scratch_chunk_bytes at a time, then their kept bins
        const size_t chunk = composed_chunk(ctx, win_len, total);
        const int rc = ensure(ctx, ctx->real_tmp, chunk * win_len * 8);
        if (rc) return rc;
        return for_chunks(total, chunk, [&](size_t t0, size_t nt) {
            return framed_produce(ctx, s, FRAMES_HALF, t0, nt, d_out + t0 * bins * 2, static_cast<cpx<float> *>(ctx->real_tmp.p));
        });
    }
    StftHalfRowsIO io{};
    fill_rows_io(io, s);
    io.out = reinterpret_cast<cpx<float> *>(d_out);
    return dispatch<float, EPI_STORE>(ctx, io, win_len, total);
}

int kofft_hip_stft_onesided_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                                size_t win_len, size_t hop, float *out, size_t frames)
{
    const int crc = stft_onesided_check(true, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (!ctx || (!signal && len) || !window || !out) return KOFFT_ERR_NULL;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, len, frames * (win_len / 2 + 1) * 2, window, win_len, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return kofft_hip_dev_stft_onesided_f32(ctx, d_in, nb, len, len, d_win, win_len, hop, d_out, frames);
                            });
}

// istft_rows_dev's mode 2 walk with the Hermitian completion in the place of its copy: d_half is never written
int kofft_hip_dev_istft_onesided_f32(kofft_hip_ctx *ctx, const float *d_half, size_t rows, size_t frames, const float *d_window,
                                     size_t win_len, size_t hop, float *d_output, size_t out_len)
{
    return istft_rows_dev(ctx, const_cast<float *>(d_half), rows, frames, d_window, win_len, hop, d_output, out_len, nullptr, out_len, 2, true,
                          true);
}

int kofft_hip_istft_onesided_f32(kofft_hip_ctx *ctx, const float *half, size_t rows, size_t frames, const float *window, size_t win_len,
                                 size_t hop, float *output, size_t out_len)
{
    const int crc = istft_rows_check(rows, frames, win_len, hop, out_len, out_len, 2);
    if (crc || rows == 0) return crc;
    // mode 2: the staged frames go up and do not come back
    return istft_stage(ctx, const_cast<float *>(half), rows, frames, window, win_len, output, out_len, nullptr, 2,
                       [&](float *d_half, const float *d_win, float *d_out, float *) {
                           return kofft_hip_dev_istft_onesided_f32(ctx, d_half, rows, frames, d_win, win_len, hop, d_out, out_len);
                       }, win_len / 2 + 1);
}

}  // extern "C"
