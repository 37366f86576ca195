// k_stft_rows.hip -- STFT (stft.rs:76-105), stft_magnitudes (visual/spectrogram.rs:52-76) and ISTFT (stft.rs:117-156, 289-343) over
// ROWS of signals on device and host pointers, with their extern "C" entry points.  Row r of every output is what k_stft.hip's single-signal entry returns for
// signal r alone; one launch chain serves all rows.  Also the framed families' shared host side: framed_src (what a framed call reads)
// and framed_produce (frames t0 .. of the flat index densely into scratch: full, their kept bins, or their magnitudes).
#include "host_common.hip.h"
#include "host_stage.hip.h"

#include "frame_cut.h"

namespace kofft {
namespace host {

// ---- composed form (window lengths the fused kernels do not cover): the framing product of transforms t0 .. of the flat index
// t = row * frames + frame into `out`, then fft_dev in place.  The twin of stft_frame_kernel.
__global__ __launch_bounds__(256) void stft_rows_frame_kernel(const float *__restrict__ signal, const float *__restrict__ window,
                                                              cpx<float> *__restrict__ out, const size_t len, const size_t row_stride,
                                                              const size_t frames, const size_t win_len, const size_t hop, const size_t t0,
                                                              const size_t total /* transforms * win_len */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t t = t0 + idx / win_len, i = idx % win_len;
    const size_t row = t / frames, f = t - row * frames;
    const size_t pos = f * hop + i;  // inside the row: a frame never reads the head of the next one
    out[idx] = mk<float>(pos < len ? signal[row * row_stride + pos] * window[i] : 0.0f, 0.0f);  // stft.rs:95-100
}

// magnitudes of bins 0 .. n/2-1 of composed frames t0 .. and each row's maximum (spectrogram.rs:63-71).  The twin of mag_kernel:
// one element per thread, whole wavefronts reach row_max_commit.
__global__ __launch_bounds__(256) void mag_rows_kernel(const cpx<float> *__restrict__ spec, float *__restrict__ mags,
                                                       unsigned *__restrict__ max_bits, const size_t frames, const size_t win_len,
                                                       const size_t t0, const size_t total /* transforms * (win_len/2) */)
{
    const size_t half = win_len / 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    float v = 0.0f;
    unsigned row = 0;
    if (idx < total) {
        const size_t t = idx / half;
        const cpx<float> c = spec[t * win_len + (idx - t * half)];
        v = sqrtf(c.re * c.re + c.im * c.im);
        mags[idx] = v;
        row = (unsigned)((t0 + t) / frames);
    }
    row_max_commit(max_bits, row, v, false);  // (`if mag > max_mag`: a NaN is never a candidate)
}

// ... without a maximum: mag_rows_kernel's values (framed_produce, FRAMES_MAGS)
__global__ __launch_bounds__(256) void frontend_mag_kernel(const cpx<float> *__restrict__ spec, float *__restrict__ mags, const size_t win_len,
                                                           const size_t total /* transforms * (win_len/2) */)
{
    const size_t half = win_len / 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t t = idx / half;
    const cpx<float> c = spec[t * win_len + (idx - t * half)];
    mags[idx] = sqrtf(c.re * c.re + c.im * c.im);
}

// composed frames -> their kept bins: dst[t][k] = src[t][k], k < bins.  One bin per thread (framed_produce, FRAMES_HALF).
__global__ __launch_bounds__(256) void pack_half_kernel(const cpx<float> *__restrict__ src, cpx<float> *__restrict__ dst, const size_t win_len,
                                                        const size_t bins, const size_t total /* transforms * bins */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t t = idx / bins, k = idx - t * bins;
    dst[idx] = src[t * win_len + k];
}

// The ordered overlap-add of istft_ola_kernel over rows: one thread per output sample of rows * out_len, the same sums in the same
// order (frames f_lo .. f_hi of the sample's OWN row, increasing f; no atomics).  MODE 1: stft::istft, MODE 2: stft::inverse_parallel.
template <int MODE>
__global__ __launch_bounds__(256) void istft_ola_rows_kernel(const cpx<float> *__restrict__ frames, const float *__restrict__ window,
                                                             float *__restrict__ output, float *__restrict__ scratch, const size_t nframes,
                                                             const size_t win_len, const size_t hop, const size_t out_len,
                                                             const size_t total /* rows * out_len */)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t row = idx / out_len, s = idx - row * out_len;
    const cpx<float> *fr = frames + row * nframes * win_len;
    float acc = output[idx];  // accumulated into the caller's buffer (stft.rs:144, 330)
    float norm = 0.0f;
    if (nframes > 0 && win_len > 0) {
        size_t f_hi = s / hop;
        if (f_hi > nframes - 1) f_hi = nframes - 1;
        const size_t f_lo = (s >= win_len) ? (s - win_len) / hop + 1 : 0;
        for (size_t f = f_lo; f <= f_hi; ++f) {
            const size_t i = s - f * hop;
            const float w = window[i];
            acc = acc + fr[f * win_len + i].re * w;
            norm = norm + w * w;
        }
    }
    if (MODE == 1) scratch[idx] = norm;
    if (norm > 1e-8f) output[idx] = acc / norm;  // stft.rs:150-154 / 335-341
    else output[idx] = (MODE == 2) ? 0.0f : acc;
}

static bool mul_ok(size_t a, size_t b, size_t *out)
{
    if (a != 0 && b > SIZE_MAX / a) return false;
    *out = a * b;
    return true;
}

int stft_rows_check(bool host_form, bool mags, size_t rows, size_t len, size_t row_stride, size_t win_len, size_t hop, size_t frames)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;  // stft.rs:83 / 242
    if (host_form || mags) {
        const size_t required = len / hop + (len % hop != 0);  // stft.rs:86
        if (frames < required) return KOFFT_ERR_MISMATCHED_LENGTHS;
    }
    if (rows == 0 || frames == 0) return KOFFT_OK;
    if (win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!complex_len_ok(win_len)) return KOFFT_ERR_UNSUPPORTED;
    if (rows > 1 && row_stride < len) return KOFFT_ERR_INVALID_VALUE;
    size_t t, e;
    if (rows > 0xffffffffULL || !mul_ok(rows, frames, &t) || !mul_ok(t, win_len, &e) || e > (SIZE_MAX >> 4)) return KOFFT_ERR_UNSUPPORTED;
    if (!mul_ok(rows, row_stride > len ? row_stride : len, &e) || e > (SIZE_MAX >> 3)) return KOFFT_ERR_UNSUPPORTED;
    return KOFFT_OK;
}

// transforms t0 .. t0 + nt of the flat index, composed (any window length): framing product into dst, fft_dev in place
static int stft_rows_composed(kofft_hip_ctx *ctx, const float *d_signal, size_t len, size_t row_stride, size_t frames, const float *d_window,
                              size_t win_len, size_t hop, cpx<float> *dst, size_t t0, size_t nt)
{
    const size_t blocks = (nt * win_len + 255) / 256;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(stft_rows_frame_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_signal, d_window, dst, len, row_stride,
                       frames, win_len, hop, t0, nt * win_len);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return fft_dev<float>(ctx, reinterpret_cast<const float *>(dst), reinterpret_cast<float *>(dst), win_len, nt, 0);
}

size_t composed_chunk(const kofft_hip_ctx *ctx, size_t win_len, size_t count)
{
    return scratch_chunk_rows(ctx->scratch_chunk_bytes, win_len * 8, count);
}

int framed_src(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len,
               size_t hop, size_t frames, FramedSrc *src)
{
    *src = FramedSrc{d_signal, d_window, rows, len, rows == 1 ? 0 : row_stride, win_len, hop, frames, fused_len_ok<float>(win_len)};
    return d_window ? KOFFT_OK : hann_table(ctx, win_len, &src->win);  // window::hann(win_len), stft_magnitudes' own
}

int framed_produce(kofft_hip_ctx *ctx, const FramedSrc &s, FramedForm form, size_t t0, size_t nt, void *dst, cpx<float> *spec)
{
    const size_t half = s.win_len / 2, per = form == FRAMES_HALF ? half + 1 : half;  // values per frame of the two packed forms
    if (!s.kernels) {
        const size_t blocks = (nt * per + 255) / 256;
        if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
        cpx<float> *frames = form == FRAMES_FULL ? static_cast<cpx<float> *>(dst) : spec;
        const int rc = stft_rows_composed(ctx, s.signal, s.len, s.row_stride, s.frames, s.win, s.win_len, s.hop, frames, t0, nt);
        if (rc || form == FRAMES_FULL) return rc;
        if (form == FRAMES_HALF)
            hipLaunchKernelGGL(pack_half_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, spec, static_cast<cpx<float> *>(dst), s.win_len,
                               per, nt * per);
        else
            hipLaunchKernelGGL(frontend_mag_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, spec, static_cast<float *>(dst), s.win_len,
                               nt * per);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return KOFFT_OK;
    }
    if (form == FRAMES_FULL) return KOFFT_ERR_UNSUPPORTED;  // (never: the full frames of these lengths are one dispatch, kofft_hip_dev_stft_rows_f32)
    FramePiece p[3];
    const int np = frame_cut(t0, nt, s.frames, p);
    for (int k = 0; k < np; ++k) {
        const float *sig = s.signal ? s.signal + p[k].row * s.row_stride : nullptr;
        const int rc = form == FRAMES_HALF ? stft_onesided_piece(ctx, sig, p[k].nr, s.len, s.row_stride, s.win, s.win_len, s.hop, p[k].f0, p[k].nf,
                                                                 static_cast<float *>(dst) + p[k].at * per * 2)
                                           : mags_piece(ctx, sig, p[k].nr, s.len, s.row_stride, s.win, s.win_len, s.hop, p[k].f0, p[k].nf,
                                                        static_cast<float *>(dst) + p[k].at * per);
        if (rc) return rc;
    }
    return KOFFT_OK;
}

// Frames per row from which a row alone is a persistent-kernel batch for StftMagIO; SIZE_MAX: never.  These are dispatch()'s f32
// thresholds (host_common.hip.h) with its conditions -- use_persist, and persist_small and group_rows_ok() below n = 512 -- and have to
// follow them; a threshold that lags behind only changes which of two routes with the same bytes runs.
static size_t mag_rows_loop_frames(const kofft_hip_ctx *ctx, size_t win_len, size_t hop)
{
    if (!ctx->use_persist) return SIZE_MAX;
    const int L = ilog2(win_len);
    const size_t cus = (size_t)ctx->num_cus;
    if (L == 12 || L == 13) return cus * 4;
    if (L == 11) return cus * 16;
    if (L == 10) return cus * 32;
    if (L == 9) return cus * 64;
    if (L >= 6 && L <= 8 && ctx->persist_small && hop <= (size_t(1) << 24)) return cus * (size_t(128) << (8 - L));
    return SIZE_MAX;
}
// ... and only for a few rows: the loop is one launch chain per row
constexpr size_t kMagRowsLoopMaxRows = 32;

int stft_mag_rows_dev(kofft_hip_ctx *ctx, const float *d_samples, size_t rows, size_t len, size_t row_stride, size_t win_len, size_t hop,
                      float *d_mags, size_t frames, float *d_max)
{
    const int crc = stft_rows_check(false, true, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0) return crc;
    // (a one-sample window has no magnitude bins: d_mags is an empty array and may be null)
    if (!ctx || !d_max || (frames && ((!d_mags && win_len >= 2) || (!d_samples && len)))) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KOFFT_HIP_TRY(ctx, hipMemsetAsync(d_max, 0, rows * sizeof(float), ctx->stream));  // every max_mag starts at 0.0
    if (frames == 0) return KOFFT_OK;
    FramedSrc s;
    int rc = framed_src(ctx, d_samples, rows, len, row_stride, nullptr, win_len, hop, frames, &s);
    if (rc) return rc;
    const size_t total = rows * frames;
    unsigned *max_bits = reinterpret_cast<unsigned *>(d_max);
    if (!s.kernels) {
        const size_t chunk = composed_chunk(ctx, win_len, total);
        rc = ensure(ctx, ctx->real_tmp, chunk * win_len * 8);
        if (rc) return rc;
        cpx<float> *spec = static_cast<cpx<float> *>(ctx->real_tmp.p);
        const size_t half = win_len / 2;
        return for_chunks(total, chunk, [&](size_t t0, size_t nt) {
            const int prc = framed_produce(ctx, s, FRAMES_FULL, t0, nt, spec, nullptr);
            if (prc || nt * half == 0) return prc;
            const size_t blocks = (nt * half + 255) / 256;  // its own tail: the magnitudes and the row maximum in one kernel
            if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(mag_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, spec, d_mags + t0 * half, max_bits, frames,
                               win_len, t0, nt * half);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
            return KOFFT_OK;
        });
    }
    // Rows long enough to reach dispatch()'s persistent kernels on their own run the single-signal kernel row by row: there the
    // maximum costs one atomicMax per wavefront and KERNEL, here one per wavefront and TRANSFORM, and with few rows those pile up on a few
    // addresses (measured, n = 1024: 8 rows x 14 063 frames 1.30 ms against the loop's 0.42; 256 x 1875 1.53 against 7.37 -- DESIGN.md 5.18).
    if (rows <= kMagRowsLoopMaxRows && frames >= mag_rows_loop_frames(ctx, win_len, hop)) {
        for (size_t r = 0; r < rows; ++r) {
            rc = stft_mag_dev(ctx, d_samples + r * s.row_stride, len, win_len, hop, d_mags + r * frames * (win_len / 2), frames, d_max + r);
            if (rc) return rc;
        }
        return KOFFT_OK;
    }
    StftMagRowsIO io{};
    fill_rows_io(io, s);
    io.mags = d_mags;
    io.max_bits = max_bits;
    return dispatch<float, EPI_STORE>(ctx, io, win_len, total);
}

int istft_rows_check(size_t rows, size_t frames, size_t win_len, size_t hop, size_t out_len, size_t scratch_len, int mode)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;                               // stft.rs:125 / 299
    if (mode == 1 && scratch_len != out_len) return KOFFT_ERR_MISMATCHED_LENGTHS;  // stft.rs:128
    if (rows == 0) return KOFFT_OK;
    if (frames > 0 && win_len == 0) return KOFFT_ERR_EMPTY_INPUT;                  // fft.ifft(&mut []) -> fft.rs:1136
    if (frames > 0 && !complex_len_ok(win_len)) return KOFFT_ERR_UNSUPPORTED;
    size_t t, e;
    if (!mul_ok(rows, frames, &t) || !mul_ok(t, win_len, &e) || e > (SIZE_MAX >> 4) || !mul_ok(rows, out_len, &e) || e > (SIZE_MAX >> 3))
        return KOFFT_ERR_UNSUPPORTED;
    return KOFFT_OK;
}

// mode 1 (istft): every frame inverse-transformed in place, output accumulated into, scratch = the window-square sums.
// mode 2 (inverse_parallel): keep_frames leaves the caller's frames alone (their inverse transforms go to the context's scratch).
// (istft_fused_kernel knows one signal only: always the two-kernel route.)
int istft_rows_dev(kofft_hip_ctx *ctx, float *d_frames, size_t rows, size_t frames, const float *d_window, size_t win_len, size_t hop,
                   float *d_output, size_t out_len, float *d_scratch, size_t scratch_len, int mode, bool keep_frames, bool half)
{
    const int crc = istft_rows_check(rows, frames, win_len, hop, out_len, scratch_len, mode);
    if (crc || rows == 0) return crc;
    if (!ctx || (frames && (!d_frames || !d_window)) || (out_len && (!d_output || (mode == 1 && !d_scratch)))) return KOFFT_ERR_NULL;
    if (half && !(keep_frames && mode == 2)) return KOFFT_ERR_INVALID_VALUE;  // (never: kofft_hip_dev_istft_onesided_f32 is the one caller)
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t in_frame = half ? (win_len / 2 + 1) * 2 : win_len * 2;  // floats of one frame as the caller holds it
    // keep_frames: whole rows at a time through at most scratch_chunk_bytes of the context's scratch (one row's frames where a row alone is
    // larger) -- copy, inverse transform, overlap-add; the rows are independent, so the sums and their order do not change
    size_t rows_per = rows;
    if (keep_frames && frames > 0) {
        rows_per = scratch_chunk_rows(ctx->scratch_chunk_bytes, frames * win_len * 8, rows);
        const int trc = ensure(ctx, ctx->rows_tmp, rows_per * frames * win_len * 8);
        if (trc) return trc;
    }
    if ((rows_per * out_len + 255) / 256 > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    for (size_t r0 = 0; r0 < rows; r0 += rows_per) {
        const size_t nr = rows - r0 < rows_per ? rows - r0 : rows_per;
        const float *time_frames = d_frames + r0 * frames * in_frame;
        if (frames > 0) {
            float *dst = d_frames + r0 * frames * in_frame;
            if (keep_frames) {
                dst = static_cast<float *>(ctx->rows_tmp.p);
                if (half) {  // the completed frames F[k] = H[k], k <= n/2; conj(H[n - k]) above
                    const int erc = expand_half(ctx, time_frames, dst, nr * frames, win_len);
                    if (erc) return erc;
                } else {
                    KOFFT_HIP_TRY(ctx, hipMemcpyAsync(dst, time_frames, nr * frames * win_len * 8, hipMemcpyDeviceToDevice, ctx->stream));
                }
            }
            const int rc = fft_dev<float>(ctx, dst, dst, win_len, nr * frames, 1);
            if (rc) return rc;
            time_frames = dst;
        }
        if (out_len == 0) continue;
        const size_t total = nr * out_len;
        const unsigned blocks = (unsigned)((total + 255) / 256);
        const cpx<float> *fr = reinterpret_cast<const cpx<float> *>(time_frames);
        float *out = d_output + r0 * out_len, *scr = d_scratch ? d_scratch + r0 * out_len : nullptr;
        if (mode == 2)
            hipLaunchKernelGGL(istft_ola_rows_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, fr, d_window, out, scr, frames, win_len, hop,
                               out_len, total);
        else
            hipLaunchKernelGGL(istft_ola_rows_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, fr, d_window, out, scr, frames, win_len, hop,
                               out_len, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

// the three arrays of istft_stage over `rows` signals
static int istft_rows_host(kofft_hip_ctx *ctx, float *frames_data, size_t rows, size_t frames, const float *window, size_t win_len, size_t hop,
                           float *output, size_t out_len, float *scratch, size_t scratch_len, int mode)
{
    const int crc = istft_rows_check(rows, frames, win_len, hop, out_len, scratch_len, mode);
    if (crc || rows == 0) return crc;
    return istft_stage(ctx, frames_data, rows, frames, window, win_len, output, out_len, scratch, mode,
                       [&](float *d_frames, const float *d_win, float *d_out, float *d_scr) {
                           return istft_rows_dev(ctx, d_frames, rows, frames, d_win, win_len, hop, d_out, out_len, d_scr, out_len, mode, false);
                       }, win_len);
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dev_stft_rows_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                const float *d_window, size_t win_len, size_t hop, float *d_out, size_t frames)
{
    const int crc = stft_rows_check(false, false, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (!ctx || (!d_signal && len) || !d_window || !d_out) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = rows * frames;
    FramedSrc s;
    (void)framed_src(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, &s);  // (the caller's window: nothing to fail)
    if (!s.kernels)  // any other window length: composed over all rows at once (BlueStftSrc knows one signal only)
        return for_chunks(total, composed_chunk(ctx, win_len, total), [&](size_t t0, size_t nt) {
            return framed_produce(ctx, s, FRAMES_FULL, t0, nt, reinterpret_cast<cpx<float> *>(d_out) + t0 * win_len, nullptr);
        });
    StftRowsIO io{};
    fill_rows_io(io, s);
    io.out = reinterpret_cast<cpx<float> *>(d_out);
    return dispatch<float, EPI_STORE>(ctx, io, win_len, total);
}

// Host rows `row_stride` apart are packed (stride len) before they travel: the gaps are not the call's to read.
int kofft_hip_stft_rows_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                            size_t win_len, size_t hop, float *out, size_t frames)
{
    const int crc = stft_rows_check(true, false, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0 || frames == 0) return crc;
    if (!ctx || (!signal && len) || !window || !out) return KOFFT_ERR_NULL;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    // a chunk of the pipeline is whole rows: no seam logic on the host
    return rows_host<float>(ctx, src, out, rows, len, frames * win_len * 2, window, win_len, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return kofft_hip_dev_stft_rows_f32(ctx, d_in, nb, len, len, d_win, win_len, hop, d_out, frames);
                            });
}

int kofft_hip_dev_stft_magnitudes_rows_f32(kofft_hip_ctx *ctx, const float *d_samples, size_t rows, size_t len, size_t row_stride,
                                           size_t win_len, size_t hop, float *d_mags, size_t frames, float *d_max)
{
    return stft_mag_rows_dev(ctx, d_samples, rows, len, row_stride, win_len, hop, d_mags, frames, d_max);
}

int kofft_hip_stft_magnitudes_rows_f32(kofft_hip_ctx *ctx, const float *samples, size_t rows, size_t len, size_t row_stride, size_t win_len,
                                       size_t hop, float *mags, size_t frames, float *max_mag)
{
    const int crc = stft_rows_check(true, true, rows, len, row_stride, win_len, hop, frames);
    if (crc || rows == 0) return crc;
    if (!ctx || !max_mag || (frames && ((!mags && win_len >= 2) || (!samples && len)))) return KOFFT_ERR_NULL;
    if (frames == 0 || win_len < 2) {  // no magnitude bins: every maximum is its starting value
        for (size_t r = 0; r < rows; ++r) max_mag[r] = 0.0f;
        return KOFFT_OK;
    }
    std::vector<float> packed;
    const float *src = pack_rows(samples, rows, len, row_stride, packed);
    // never zero-copy: the maxima are atomicMax targets and stay in device memory, as in the single-signal form (k_stft.hip)
    const HostArray<float> a[3] = {{src, nullptr, len}, {nullptr, mags, frames * (win_len / 2)}, {nullptr, max_mag, 1}};
    return rows_host_n<float>(ctx, rows, 3, a, nullptr, 0, false, true, [&](float *const *d, const float *, size_t nb) {
        return stft_mag_rows_dev(ctx, d[0], nb, len, len, win_len, hop, d[1], frames, d[2]);
    });
}

int kofft_hip_dev_istft_rows_f32(kofft_hip_ctx *ctx, float *d_frames, size_t rows, size_t frames, const float *d_window, size_t win_len,
                                 size_t hop, float *d_output, size_t out_len, float *d_scratch, size_t scratch_len)
{
    return istft_rows_dev(ctx, d_frames, rows, frames, d_window, win_len, hop, d_output, out_len, d_scratch, scratch_len, 1, false);
}

int kofft_hip_dev_istft_parallel_rows_f32(kofft_hip_ctx *ctx, const float *d_frames, size_t rows, size_t frames, const float *d_window,
                                          size_t win_len, size_t hop, float *d_output, size_t out_len)
{
    return istft_rows_dev(ctx, const_cast<float *>(d_frames), rows, frames, d_window, win_len, hop, d_output, out_len, nullptr, out_len, 2,
                          true);
}

int kofft_hip_istft_rows_f32(kofft_hip_ctx *ctx, float *frames_data, size_t rows, size_t frames, const float *window, size_t win_len,
                             size_t hop, float *output, size_t out_len, float *scratch, size_t scratch_len)
{
    return istft_rows_host(ctx, frames_data, rows, frames, window, win_len, hop, output, out_len, scratch, scratch_len, 1);
}

int kofft_hip_istft_parallel_rows_f32(kofft_hip_ctx *ctx, const float *frames_data, size_t rows, size_t frames, const float *window,
                                      size_t win_len, size_t hop, float *output, size_t out_len)
{
    return istft_rows_host(ctx, const_cast<float *>(frames_data), rows, frames, window, win_len, hop, output, out_len, nullptr, out_len, 2);
}

}  // extern "C"
