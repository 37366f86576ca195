// kofft_hip.hip -- host-pointer wrappers (staging, pipelining, zero-copy) and the extern "C" ABI of
// include/kofft_hip.h.  The kernels live in the k_*.hip translation units (host_common.hip.h).
#include "host_common.hip.h"
#include "host_layout.h"
#include "resample_plan.h"
#include "sosfilt_plan.h"

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>

using namespace kofft;
using namespace kofft::host;

namespace {

// Large host batches: the transfers dominate (the kernel is ~100 x shorter than its PCIe time), so the batch goes through
// in chunks with the upload of chunk c+1, the kernel of chunk c and the download of chunk c-1 in flight together.
// Uploads and kernels are issued from the calling thread, downloads from a helper thread (a pageable-memory copy blocks
// its caller), each on its own stream; events order them.  Transforms are independent, so chunking cannot change a
// result.  Measured, 8192 x 4096 c32 from pageable memory: 9.6 -> 7.0 ms (55 -> 77 GB/s over PCIe).
//   up(c, stream)   -> hipError_t : enqueue chunk c's host-to-device copy on `stream`
//   run(c)          -> int        : launch chunk c's kernels on ctx->stream (status code)
//   down(c, stream) -> hipError_t : enqueue chunk c's device-to-host copy on `stream`
template <class Up, class Run, class Down>
int pipeline_chunks(kofft_hip_ctx *ctx, size_t nchunks, Up up, Run run, Down down)
{
    // KOFFT_ERR_ALLOC from here = "could not set the pipeline up": the caller takes the serial path instead.
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> uploaded(nchunks, nullptr), done(nchunks, nullptr);
    auto cleanup = [&]() {
        for (size_t c = 0; c < nchunks; ++c) {
            if (uploaded[c]) (void)hipEventDestroy(uploaded[c]);
            if (done[c]) (void)hipEventDestroy(done[c]);
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        if (s_out) (void)hipStreamDestroy(s_out);
    };
    bool ok = hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking) == hipSuccess;
    for (size_t c = 0; c < nchunks && ok; ++c)
        ok = hipEventCreateWithFlags(&uploaded[c], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&done[c], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        cleanup();
        return KOFFT_ERR_ALLOC;
    }
    // hand-off to the download thread: chunks [0, launched) have their kernels enqueued and `done` recorded
    std::mutex mu;
    std::condition_variable cv;
    size_t launched = 0;
    bool failed = false;
    const int device = ctx->device;
    std::thread downloader;
    try {
        downloader = std::thread([&]() {
            (void)hipSetDevice(device);
            for (size_t c = 0; c < nchunks; ++c) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return launched > c || failed; });
                    if (failed) return;
                }
                if (hipEventSynchronize(done[c]) != hipSuccess || down(c, s_out) != hipSuccess ||
                    hipStreamSynchronize(s_out) != hipSuccess) {
                    std::lock_guard<std::mutex> lk(mu);
                    failed = true;
                    return;
                }
            }
        });
    } catch (...) {  // no helper thread available
        cleanup();
        return KOFFT_ERR_ALLOC;
    }
    auto has_failed = [&] {
        std::lock_guard<std::mutex> lk(mu);
        return failed;
    };
    int rc = KOFFT_OK;
    for (size_t c = 0; c < nchunks && rc == KOFFT_OK && !has_failed(); ++c) {
        if (up(c, s_in) != hipSuccess || hipEventRecord(uploaded[c], s_in) != hipSuccess ||
            hipStreamWaitEvent(ctx->stream, uploaded[c], 0) != hipSuccess) {
            rc = KOFFT_ERR_HIP;
            ctx->last_error = "pipelined upload failed";
            break;
        }
        rc = run(c);
        if (rc == KOFFT_OK && hipEventRecord(done[c], ctx->stream) != hipSuccess) rc = KOFFT_ERR_HIP;
        if (rc == KOFFT_OK) {
            {
                std::lock_guard<std::mutex> lk(mu);
                launched = c + 1;
            }
            cv.notify_one();
        }
    }
    bool dl_failed;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (rc != KOFFT_OK) failed = true;
        dl_failed = failed;
    }
    cv.notify_one();
    downloader.join();
    {
        std::lock_guard<std::mutex> lk(mu);
        dl_failed = failed;
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(s_in);
    cleanup();
    // On failure the caller's buffers hold a mix of transformed and untouched chunks (in-place entry points): a
    // negative status means "contents undefined", as for any HIP failure.
    if (rc == KOFFT_OK && dl_failed) {
        rc = KOFFT_ERR_HIP;
        ctx->last_error = "pipelined download failed";
    }
    return rc;
}

// does a host batch of `bytes` (both directions together) in `batch` independent rows, `row_bytes` in the smallest row of an array that
// travels, go through the pipeline?
inline bool use_host_pipeline(const kofft_hip_ctx *ctx, size_t bytes, size_t batch, size_t row_bytes)
{
    return ctx->host_pipeline && bytes >= (size_t(128) << 20) && batch >= 16 && row_bytes <= (size_t(8) << 20);
}

// One array of a host-pointer call: `row` elements of T per row (0: an empty array).  `up` is copied to the device before the work,
// `down` receives the device's copy after it -- the same pointer for an array transformed in place, both null for device-only space.
template <typename T>
struct HostArray {
    const T *up;
    T *down;
    size_t row;
};

// The one way a host-pointer call reaches the device: `batch` independent rows of n <= kMaxHostArrays arrays, and an optional side
// input of side_len elements that every row reads (rfft's window, the Goertzel coefficients), uploaded once.  The arrays and the side
// input lie in one buffer as host_layout() places them; dev(d, d_side, rows) enqueues the device work for `rows` rows on ctx->stream,
// d[k] pointing at array k's first row (never null, also for an empty array).  Three ways through:
//  * zero-copy, when the caller's own rule allows it (`zero_copy`) and the context does: the buffer is the pinned, device-mapped one,
//    which the kernels read and write over PCIe;
//  * pipelined (use_host_pipeline, when pipeline_ok; every array's rows must be contiguous): pipeline_chunks over the staged device
//    buffer, chunk c of array k being its rows [c * chunk, ...), the side input uploaded ahead of the chunks;
//  * serial: upload (the arrays, then the side input: a small copy queued ahead of the large ones costs a staged call of a few MiB
//    about 12 us), device work, download through the staged device buffer.
template <typename T, class Dev>
int stage_host(kofft_hip_ctx *ctx, size_t batch, int n, const HostArray<T> *a, const T *side, size_t side_len, bool zero_copy,
               bool pipeline_ok, Dev dev)
{
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t row[kMaxHostArrays];
    for (int k = 0; k < n; ++k) row[k] = a[k].row;
    const size_t side_bytes = side ? side_len * sizeof(T) : 0;
    const HostLayout lay = host_layout(n, row, batch, sizeof(T), side_bytes);
    auto bytes = [&](int k) { return batch * row[k] * sizeof(T); };
    T *d[kMaxHostArrays];
    auto point_at = [&](void *base) {  // -> the side input there
        for (int k = 0; k < n; ++k) d[k] = reinterpret_cast<T *>(static_cast<char *>(base) + lay.off[k]);
        return side ? reinterpret_cast<const T *>(static_cast<char *>(base) + lay.side) : nullptr;
    };
    if (zero_copy && ctx->zero_copy && ensure_pinned(ctx, lay.total) == KOFFT_OK) {
        char *h = static_cast<char *>(ctx->pinned);
        for (int k = 0; k < n; ++k)
            if (a[k].up && bytes(k)) std::memcpy(h + lay.off[k], a[k].up, bytes(k));
        if (side_bytes) std::memcpy(h + lay.side, side, side_bytes);
        const T *d_side = point_at(ctx->pinned_dev);
        const int zrc = dev(d, d_side, batch);
        if (zrc) return zrc;
        KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < n; ++k)
            if (a[k].down && bytes(k)) std::memcpy(a[k].down, h + lay.off[k], bytes(k));
        return KOFFT_OK;
    }
    int rc = ensure(ctx, ctx->stage, lay.total);
    if (rc) return rc;
    const T *d_side = point_at(ctx->stage.p);
    auto side_up = [&] { return side_bytes ? hipMemcpyAsync(const_cast<T *>(d_side), side, side_bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess; };
    // rows [r0, r0 + nr) of every array that travels in this direction
    auto copy_rows = [&](bool up, size_t r0, size_t nr, hipStream_t st) {
        for (int k = 0; k < n; ++k) {
            const size_t at = r0 * row[k], nb = nr * row[k] * sizeof(T);
            hipError_t e = hipSuccess;
            if (up && a[k].up && nb) e = hipMemcpyAsync(d[k] + at, a[k].up + at, nb, hipMemcpyHostToDevice, st);
            if (!up && a[k].down && nb) e = hipMemcpyAsync(a[k].down + at, d[k] + at, nb, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    size_t moved = 0, min_row = SIZE_MAX;
    for (int k = 0; k < n; ++k) {
        if (!a[k].up && !a[k].down) continue;
        moved += ((a[k].up ? 1 : 0) + (a[k].down ? 1 : 0)) * bytes(k);
        min_row = std::min(min_row, row[k]);
    }
    if (pipeline_ok && use_host_pipeline(ctx, moved, batch, min_row * sizeof(T))) {
        KOFFT_HIP_TRY(ctx, side_up());
        constexpr int kHostChunks = 8;  // pieces of a pipelined host batch
        const size_t chunk = host_chunk_rows(batch, kHostChunks);
        auto rows = [&](size_t c) { return (batch - c * chunk < chunk) ? batch - c * chunk : chunk; };
        const int prc = pipeline_chunks(
            ctx, (batch + chunk - 1) / chunk, [&](size_t c, hipStream_t st) { return copy_rows(true, c * chunk, rows(c), st); },
            [&](size_t c) {
                T *dc[kMaxHostArrays];
                for (int k = 0; k < n; ++k) dc[k] = d[k] + c * chunk * row[k];
                return dev(dc, d_side, rows(c));
            },
            [&](size_t c, hipStream_t st) { return copy_rows(false, c * chunk, rows(c), st); });
        if (prc != KOFFT_ERR_ALLOC) return prc;  // (no helper thread: serial path below)
    }
    KOFFT_HIP_TRY(ctx, copy_rows(true, 0, batch, ctx->stream));
    KOFFT_HIP_TRY(ctx, side_up());
    rc = dev(d, d_side, batch);
    if (rc) return rc;
    KOFFT_HIP_TRY(ctx, copy_rows(false, 0, batch, ctx->stream));
    KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KOFFT_OK;
}

// stage_host under the row-wise entry points' zero-copy rule: neither direction (up-arrays + side input, down-arrays) above kZeroCopyMax
template <typename T, class Dev>
int rows_host_n(kofft_hip_ctx *ctx, size_t batch, int n, const HostArray<T> *a, const T *side, size_t side_len, bool zero_copy_ok,
                bool pipeline_ok, Dev dev)
{
    size_t up = side ? side_len * sizeof(T) : 0, down = 0;
    for (int k = 0; k < n; ++k) {
        if (a[k].up) up += batch * a[k].row * sizeof(T);
        if (a[k].down) down += batch * a[k].row * sizeof(T);
    }
    return stage_host<T>(ctx, batch, n, a, side, side_len, zero_copy_ok && std::max(up, down) <= kZeroCopyMax, pipeline_ok, dev);
}

// rows_host_n with one input and one output array: dev(d_in, d_out, d_side, rows)
template <typename T, class Dev>
int rows_host(kofft_hip_ctx *ctx, const T *in, T *out, size_t batch, size_t in_row, size_t out_row, const T *side, size_t side_len,
              bool zero_copy_ok, bool pipeline_ok, Dev dev)
{
    const HostArray<T> a[2] = {{in, nullptr, in_row}, {nullptr, out, out_row}};
    return rows_host_n<T>(ctx, batch, 2, a, side, side_len, zero_copy_ok, pipeline_ok,
                          [&](T *const *d, const T *d_side, size_t rows) { return dev(d[0], d[1], d_side, rows); });
}

template <typename T>
int fft_host(kofft_hip_ctx *ctx, T *data, size_t n, size_t batch, int inverse)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n > (size_t(1) << (is_pow2(n) ? max_log2_big<T>() : max_log2_big<T>() - 1))) return KOFFT_ERR_UNSUPPORTED;
    if (n == 1) return KOFFT_OK;
    if (!ctx || !data) return KOFFT_ERR_NULL;
    const HostArray<T> a{data, data, 2 * n};
    return rows_host_n<T>(ctx, batch, 1, &a, nullptr, 0, is_pow2(n), true,
                          [&](T *const *d, const T *, size_t rows) { return fft_dev<T>(ctx, d[0], d[0], n, rows, inverse); });
}

// FftImpl::fft_split / ifft_split on host planes of batch * n reals each, in place (planar_impl.hip.h)
template <typename T>
int planar_host(kofft_hip_ctx *ctx, T *re, T *im, size_t n, size_t batch, int inverse)
{
    const int rc = planar_check(n, batch, re, im, re, im, ctx);
    if (rc || batch == 0) return rc;
    if (n == 1) return KOFFT_OK;  // the planes themselves
    const HostArray<T> a[2] = {{re, re, n}, {im, im, n}};
    return rows_host_n<T>(ctx, batch, 2, a, nullptr, 0, is_pow2(n), true,
                          [&](T *const *d, const T *, size_t nb) { return planar_dev<T>(ctx, d[0], d[1], d[0], d[1], n, nb, inverse); });
}

// ScalarFftImpl::fft_radix4 on a host buffer (fft_radix4.hip.h); inverse: FftPlan::ifft's loop around it (fft.rs:2040-2055)
template <typename T>
int fft_radix4_host(kofft_hip_ctx *ctx, T *data, size_t n, size_t batch, int inverse)
{
    if (batch == 0) return KOFFT_OK;
    if (!is_pow2(n) || (ilog2(n) & 1)) return fft_host<T>(ctx, data, n, batch, inverse);  // fft.rs:1457-1460
    if (n > (size_t(1) << max_log2_big<T>())) return KOFFT_ERR_UNSUPPORTED;
    if (n == 1) return KOFFT_OK;
    if (!ctx || !data) return KOFFT_ERR_NULL;
    const HostArray<T> a{data, data, 2 * n};
    return stage_host<T>(ctx, batch, 1, &a, nullptr, 0, false, false,
                         [&](T *const *d, const T *, size_t rows) { return fft_radix4_dev<T>(ctx, d[0], d[0], n, rows, inverse); });
}

// fft_strided / ifft_strided (fft.rs:1175-1199, 1236-1260): gather, transform, scatter.
template <typename T>
int fft_strided_host(kofft_hip_ctx *ctx, T *data, size_t data_len, size_t stride, size_t n, int inverse)
{
    if (stride == 0) return KOFFT_ERR_INVALID_STRIDE;  // fft.rs:1181
    if (n == 0) return KOFFT_OK;                       // fft.rs:1185
    if (data_len < (n - 1) * stride + 1) return KOFFT_ERR_MISMATCHED_LENGTHS;  // fft.rs:1188
    if (!ctx || !data) return KOFFT_ERR_NULL;
    std::vector<T> scratch(2 * n);
    for (size_t i = 0; i < n; ++i) {
        scratch[2 * i] = data[2 * i * stride];
        scratch[2 * i + 1] = data[2 * i * stride + 1];
    }
    int rc = fft_host<T>(ctx, scratch.data(), n, 1, inverse);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        data[2 * i * stride] = scratch[2 * i];
        data[2 * i * stride + 1] = scratch[2 * i + 1];
    }
    return KOFFT_OK;
}

template <typename T>
int rfft_host(kofft_hip_ctx *ctx, const T *in, T *out, const T *window, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n % 2 != 0) return KOFFT_ERR_INVALID_VALUE;
    const size_t m = n / 2;
    if (!complex_len_ok(m)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return rows_host<T>(ctx, in, out, batch, n, (m + 1) * 2, window, n, true, true,
                        [&](T *d_in, T *d_out, const T *d_win, size_t rows) { return rfft_dev<T>(ctx, d_in, d_out, d_win, n, rows); });
}

// DctPlanner::plan_dct2 on host rows of n reals in and out
int dct2_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!complex_len_ok(n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return dct2_dev(ctx, d_in, d_out, n, rows); });
}

// hilbert::hilbert_analytic on host rows of n reals in, n complex out
int hilbert_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return rows_host<float>(ctx, in, out, batch, n, 2 * n, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return hilbert_dev(ctx, d_in, d_out, n, rows); });
}

// cepstrum::real_cepstrum on host rows of n reals in and out
int cepstrum_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!is_pow2(n)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (n > (size_t(1) << max_log2_big<float>())) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return cepstrum_dev(ctx, d_in, d_out, n, rows); });
}

// overlap-save convolution / correlation on host rows: nx samples in, out_len values out (k_convolve_f32.hip).  One filter for all
// rows is the side input, uploaded once; one filter per row is a third array, so that a pipelined chunk carries its own rows' taps
int convolve_host(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh, size_t block,
                  unsigned flags, float *out, size_t out_first, size_t out_len)
{
    const int rc = convolve_check(rows, nx, nh, filters, &block, flags, out_first, out_len, x, h, out, ctx);
    if (rc || rows == 0 || out_len == 0) return rc;
    if (filters == rows && rows > 1) {
        const HostArray<float> a[3] = {{x, nullptr, nx}, {h, nullptr, nh}, {nullptr, out, out_len}};
        return rows_host_n<float>(ctx, rows, 3, a, nullptr, 0, true, true, [&](float *const *d, const float *, size_t nr) {
            return convolve_dev(ctx, d[0], nr, nx, d[1], nr, nh, block, flags, d[2], out_first, out_len);
        });
    }
    return rows_host<float>(ctx, x, out, rows, nx, out_len, h, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return convolve_dev(ctx, d_in, nr, nx, d_h, 1, nh, block, flags, d_out, out_first, out_len);
                            });
}

// the same against a bank of filters (k_convolve_f32.hip): the bank is the side input, uploaded once; a row of the
// output is filters * out_len elements of one or (complex values) two floats
int convolve_bank_host(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh, size_t block,
                       unsigned flags, void *out, size_t out_first, size_t out_len)
{
    const int rc = convolve_bank_check(rows, nx, filters, nh, &block, flags, out_first, out_len, x, h, out, ctx);
    if (rc || rows == 0 || filters == 0 || out_len == 0) return rc;
    if (filters > (SIZE_MAX >> 3) / nh || filters > (SIZE_MAX >> 3) / out_len) return KOFFT_ERR_UNSUPPORTED;
    const size_t out_row = filters * out_len * (((flags >> 2) & 3u) == 1u ? 2 : 1), side_len = filters * nh * ((flags & 2u) ? 2 : 1);
    return rows_host<float>(ctx, x, static_cast<float *>(out), rows, nx, out_row, h, side_len, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return convolve_bank_dev(ctx, d_in, nr, nx, d_h, filters, nh, block, flags, d_out, out_first, out_len);
                            });
}

// cepstrum::mel_filterbank / mfcc on host rows of n_fft magnitudes in, num_mel energies or num_coeffs coefficients out (k_mfcc_f32.hip);
// the edges stay on the host
int mel_host(kofft_hip_ctx *ctx, bool mfcc, const float *mags, float *out, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
             size_t num_coeffs)
{
    const int rc = mel_check(mfcc, false, mags, out, n_fft, rows, bins, num_mel, num_coeffs, ctx);
    if (rc || rows == 0 || num_mel == 0 || (mfcc && num_coeffs == 0)) return rc;
    return rows_host<float>(ctx, mags, out, rows, n_fft, mfcc ? num_coeffs : num_mel, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t nr) {
                                return mfcc ? mfcc_dev(ctx, d_in, d_out, n_fft, nr, bins, num_mel, num_coeffs)
                                            : mel_filterbank_dev(ctx, d_in, d_out, n_fft, nr, bins, num_mel);
                            });
}

// visual::spectrogram's magnitude_to_db (which == 0) / db_scale on `count` host magnitudes, max_mag a host float (k_spectrogram_f32.hip):
// one row of `count` values with max_mag as the side input
int spec_db_host(kofft_hip_ctx *ctx, int which, const float *mags, size_t count, const float *max_mag, float level, float *out)
{
    const int rc = spec_db_check(false, mags, count, max_mag, out, ctx);
    if (rc) return rc;
    return rows_host<float>(ctx, mags, out, 1, count, count, max_mag, 1, true, true,
                            [&](float *d_in, float *d_out, const float *d_max, size_t) { return spec_db_dev(ctx, which, d_in, count, d_max, level, d_out); });
}

// the render on a host picture: the magnitudes and the picture travel as bytes (one row each), max_mag as the side input; the table
// stays on the host
int spec_render_host(kofft_hip_ctx *ctx, const float *mags, size_t frames, size_t bins, const float *max_mag, int mode, float level, int cmap,
                     int depth, int scale, int layout, const uint32_t *pix_of_bin, void *out)
{
    const int rc = spec_render_check(false, mags, frames, bins, max_mag, mode, cmap, depth, scale, layout, pix_of_bin, out, ctx);
    if (rc) return rc;
    typedef unsigned char byte;
    return rows_host<byte>(ctx, reinterpret_cast<const byte *>(mags), static_cast<byte *>(out), 1, frames * bins * sizeof(float),
                           frames * bins * (depth == 16 ? 6 : 3), reinterpret_cast<const byte *>(max_mag), sizeof(float), true, true,
                           [&](byte *d_in, byte *d_out, const byte *d_max, size_t) {
                               return spec_render_dev(ctx, reinterpret_cast<const float *>(d_in), frames, bins, reinterpret_cast<const float *>(d_max),
                                                      mode, level, cmap, depth, scale, layout, pix_of_bin, d_out);
                           });
}

// dct::dct1..4 / dst::dst1..4 on host rows of n reals in and out
int direct_host(kofft_hip_ctx *ctx, int family, int type, const float *in, float *out, size_t n, size_t batch)
{
    int rc = direct_check(family, type, n, batch, in, out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    // No pipeline: the whole input is on the device before any output is written back, so in == out works (the reference's
    // batch_* are in place).
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, false,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return direct_dev(ctx, family, type, d_in, d_out, n, rows); });
}

// hartley::dht on host rows of n reals in and out (k_hartley_f32.hip)
int dht_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    int rc = dht_check(n, batch, in, out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    // No pipeline, like direct_host: in == out works (hartley::batch is in place).
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, false,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return dht_dev(ctx, d_in, d_out, n, rows); });
}

// czt::czt_f32 on host rows: n reals in, m complex out (k_spectral_f32.hip)
int czt_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t m, float wr, float wi, float ar, float ai, size_t batch)
{
    int rc = czt_check(n, m, batch, in, out, ctx);
    if (rc || batch == 0 || m == 0) return rc;
    if (n == 0) {  // the loop body never runs: (+0, +0) in every bin
        std::memset(out, 0, batch * 2 * m * sizeof(float));
        return KOFFT_OK;
    }
    return rows_host<float>(ctx, in, out, batch, n, 2 * m, nullptr, 0, true, false,
                            [&](float *d_in, float *d_out, const float *, size_t rows) { return czt_dev(ctx, d_in, d_out, n, m, wr, wi, ar, ai, rows); });
}

// goertzel::goertzel_f32 on host rows against nfreq frequencies: the coefficients go up as the side input
int goertzel_host(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch, float sample_rate, const float *target_freqs,
                  size_t nfreq)
{
    int rc = goertzel_check(n, batch, sample_rate, target_freqs, nfreq, in, out, ctx);
    if (rc || batch == 0 || nfreq == 0) return rc;
    std::vector<float> coeff(nfreq);
    kofft_tables::goertzel_coeff_f32(n, sample_rate, target_freqs, nfreq, coeff.data());
    return rows_host<float>(ctx, in, out, batch, n, nfreq, coeff.data(), nfreq, true, true,
                            [&](float *d_in, float *d_out, const float *d_coeff, size_t rows) { return goertzel_launch(ctx, d_in, d_out, d_coeff, n, rows, nfreq); });
}

// wavelet::*_forward / *_inverse (one level) and multi_level_forward / _inverse on host rows (k_wavelet_f32.hip)
int dwt_host(kofft_hip_ctx *ctx, int w, const float *in, float *approx, float *detail, size_t len, size_t batch)
{
    int rc = dwt_check(w, len, batch, 0, in, approx, detail, ctx);
    if (rc || batch == 0 || len / 2 == 0) return rc;
    const HostArray<float> a[3] = {{in, nullptr, len}, {nullptr, approx, len / 2}, {nullptr, detail, len / 2}};
    return rows_host_n<float>(ctx, batch, 3, a, nullptr, 0, true, true,
                              [&](float *const *d, const float *, size_t rows) { return dwt_dev(ctx, w, d[0], d[1], d[2], len, rows); });
}

int idwt_host(kofft_hip_ctx *ctx, int w, const float *approx, const float *detail, float *out, size_t n, size_t batch)
{
    const size_t one = n;
    int rc = idwt_check(w, n, batch, 1, &one, approx, detail, out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    const HostArray<float> a[3] = {{approx, nullptr, n}, {detail, nullptr, n}, {nullptr, out, 2 * n}};
    return rows_host_n<float>(ctx, batch, 3, a, nullptr, 0, true, true,
                              [&](float *const *d, const float *, size_t rows) { return idwt_dev(ctx, w, d[0], d[1], d[2], n, rows); });
}

// (the details are packed level after level, [batch][a_l] each: not row-contiguous, so no pipeline)
int dwt_multi_host(kofft_hip_ctx *ctx, int w, const float *in, float *approx, float *details, size_t len, size_t batch, size_t levels)
{
    int rc = dwt_check(w, len, batch, levels, in, approx, levels ? details : approx, ctx);
    if (rc || batch == 0 || len == 0) return rc;
    size_t lens[kWaveletMaxLevels + 1];
    const size_t det = wavelet_lengths(len, levels, lens);
    const HostArray<float> a[3] = {{in, nullptr, len}, {nullptr, approx, lens[levels]}, {nullptr, details, det}};
    return rows_host_n<float>(ctx, batch, levels ? 3 : 2, a, nullptr, 0, true, false, [&](float *const *d, const float *, size_t rows) {
        return dwt_multi_dev(ctx, w, d[0], d[1], levels ? d[2] : nullptr, len, rows, levels);
    });
}

int idwt_multi_host(kofft_hip_ctx *ctx, int w, const float *approx, const float *details, const size_t *detail_lens, float *out, size_t n,
                    size_t batch, size_t levels)
{
    int rc = idwt_check(w, n, batch, levels, detail_lens, approx, levels ? details : approx, out, ctx);
    if (rc || batch == 0 || n == 0) return rc;
    size_t det = 0;
    for (size_t l = 0; l < levels; ++l) det += detail_lens[l];
    const HostArray<float> a[3] = {{approx, nullptr, n}, {nullptr, out, n << levels}, {details, nullptr, det}};
    return rows_host_n<float>(ctx, batch, levels ? 3 : 2, a, nullptr, 0, true, false, [&](float *const *d, const float *, size_t rows) {
        return idwt_multi_dev(ctx, w, d[0], levels ? d[2] : nullptr, detail_lens, d[1], n, rows, levels);
    });
}

template <typename T>
int irfft_host(kofft_hip_ctx *ctx, const T *in, T *out, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n % 2 != 0) return KOFFT_ERR_INVALID_VALUE;
    const size_t m = n / 2;
    if (!complex_len_ok(m)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return rows_host<T>(ctx, in, out, batch, (m + 1) * 2, n, nullptr, 0, true, true,
                        [&](T *d_in, T *d_out, const T *, size_t rows) { return irfft_dev<T>(ctx, d_in, d_out, n, rows); });
}

// Host-pointer STFT of frames starting at start0, start0+hop, ...: uploads only the samples
// those frames can see.
int stft_host(kofft_hip_ctx *ctx, const float *signal, size_t len, const float *window, size_t win_len,
              size_t start0, size_t hop, float *out, size_t count)
{
    if (count == 0) return KOFFT_OK;
    if (win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!complex_len_ok(win_len)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || (!signal && len) || !window || !out) return KOFFT_ERR_NULL;
    const size_t lo = start0 < len ? start0 : len;
    size_t hi = start0 + (count - 1) * hop + win_len;
    if (hi > len) hi = len;
    if (hi < lo) hi = lo;
    const size_t span = hi - lo;
    const size_t out_bytes = count * win_len * 2 * sizeof(float);
    const HostArray<float> a[2] = {{signal + lo, nullptr, span}, {nullptr, out, count * win_len * 2}};
    // frame() / StftStream / short signals go zero-copy.  Positions are relative to `lo`; a start past the end of the signal leaves
    // every sample zero.
    return stage_host<float>(ctx, 1, 2, a, window, win_len, (span + win_len) * sizeof(float) + out_bytes <= kZeroCopyMax, false,
                             [&](float *const *d, const float *d_win, size_t) {
                                 return stft_dev(ctx, d[0], span, d_win, win_len, start0 - lo, hop, d[1], count);
                             });
}

// The three arrays of a host-pointer ISTFT over `rows` signals (1: istft / inverse_parallel / inverse_frame): the frames go up and, unless
// mode 2 (inverse_parallel clones each frame, stft.rs:310: the caller's stay untouched), come back inverse-transformed; the output goes
// up and comes back; the window-square sums only come back (mode 1) or stay on the device.  dev(d_frames, d_window, d_output, d_scratch).
// bins: complex values per frame as the caller holds them -- win_len, or win_len / 2 + 1 for one-sided frames (mode 2).
template <class Dev>
int istft_stage(kofft_hip_ctx *ctx, float *frames_data, size_t rows, size_t frames, const float *window, size_t win_len, float *output,
                size_t out_len, float *scratch, int mode, Dev dev, size_t bins)
{
    if (!ctx || (frames && (!frames_data || !window)) || (out_len && (!output || (mode == 1 && !scratch)))) return KOFFT_ERR_NULL;
    const size_t fr_bytes = rows * frames * bins * 2 * sizeof(float), o_bytes = rows * out_len * sizeof(float);
    auto align = [](size_t b) { return (b + 255) & ~size_t(255); };
    // one frame (IstftStream, inverse_frame) or a short batch goes zero-copy
    const size_t total = align(fr_bytes) + 2 * align(o_bytes) + win_len * sizeof(float) + 256;
    const HostArray<float> a[3] = {{frames_data, mode == 2 ? nullptr : frames_data, frames * bins * 2},
                                   {output, output, out_len},
                                   {nullptr, mode == 1 ? scratch : nullptr, out_len}};
    return stage_host<float>(ctx, rows, 3, a, window, win_len, total <= kZeroCopyMax, false,
                             [&](float *const *d, const float *d_win, size_t) { return dev(d[0], d_win, d[1], d[2]); });
}

int istft_host(kofft_hip_ctx *ctx, float *frames_data, size_t frames, const float *window, size_t win_len, size_t hop, float *output,
               size_t out_len, float *scratch, size_t scratch_len, int mode, size_t start0)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;
    if (mode == 1 && scratch_len != out_len) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (frames > 0 && win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (frames > 0 && !complex_len_ok(win_len)) return KOFFT_ERR_UNSUPPORTED;
    return istft_stage(ctx, frames_data, 1, frames, window, win_len, output, out_len, scratch, mode,
                       [&](float *d_frames, const float *d_win, float *d_out, float *d_scr) {
                           return istft_dev(ctx, d_frames, frames, d_win, win_len, hop, d_out, out_len, d_scr, out_len, mode, start0);
                       }, win_len);
}

int istft_rows_host(kofft_hip_ctx *ctx, float *frames_data, size_t rows, size_t frames, const float *window, size_t win_len, size_t hop,
                    float *output, size_t out_len, float *scratch, size_t scratch_len, int mode)
{
    const int crc = istft_rows_check(rows, frames, win_len, hop, out_len, scratch_len, mode);
    if (crc || rows == 0) return crc;
    return istft_stage(ctx, frames_data, rows, frames, window, win_len, output, out_len, scratch, mode,
                       [&](float *d_frames, const float *d_win, float *d_out, float *d_scr) {
                           return istft_rows_dev(ctx, d_frames, rows, frames, d_win, win_len, hop, d_out, out_len, d_scr, out_len, mode, false);
                       }, win_len);
}

template <typename T>
int fft_nd_host(kofft_hip_ctx *ctx, T *data, size_t depth, size_t rows, size_t cols, int inverse)
{
    if (depth == 0 || rows == 0 || cols == 0) return KOFFT_OK;
    for (size_t n : {depth, rows, cols})
        if (!complex_len_ok(n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !data) return KOFFT_ERR_NULL;
    const HostArray<T> a{data, data, 2 * depth * rows * cols};
    return stage_host<T>(ctx, 1, 1, &a, nullptr, 0, false, false,
                         [&](T *const *d, const T *, size_t) { return fft_nd_dev<T>(ctx, d[0], depth, rows, cols, inverse); });
}

}  // namespace

// ---------------------------------------------------------------------------------
// extern "C"
// ---------------------------------------------------------------------------------
extern "C" {

const char *kofft_hip_strerror(int status)
{
    switch (status) {
    case KOFFT_OK: return "Ok";
    case KOFFT_ERR_EMPTY_INPUT: return "FftError::EmptyInput";
    case KOFFT_ERR_NON_POWER_OF_TWO_NO_STD: return "FftError::NonPowerOfTwoNoStd";
    case KOFFT_ERR_MISMATCHED_LENGTHS: return "FftError::MismatchedLengths";
    case KOFFT_ERR_INVALID_STRIDE: return "FftError::InvalidStride";
    case KOFFT_ERR_INVALID_HOP_SIZE: return "FftError::InvalidHopSize";
    case KOFFT_ERR_INVALID_VALUE: return "FftError::InvalidValue";
    case KOFFT_ERR_HIP: return "HIP runtime error (see kofft_hip_last_error)";
    case KOFFT_ERR_UNSUPPORTED: return "length not supported by the device path";
    case KOFFT_ERR_NULL: return "null context or pointer";
    case KOFFT_ERR_ALLOC: return "allocation failed";
    case KOFFT_ERR_RCCL: return "RCCL unavailable or collective failed (see kofft_hip_multi_last_error)";
    default: return "unknown status";
    }
}

const char *kofft_hip_last_error(const kofft_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

const char *kofft_hip_version(void) { return "kofft-hip 0.1.0 (gfx950)"; }

int kofft_hip_device_count(int *count)
{
    if (!count) return KOFFT_ERR_NULL;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return e == hipSuccess ? KOFFT_OK : KOFFT_ERR_HIP;
}

int kofft_hip_create(int device, kofft_hip_ctx **out)
{
    if (!out) return KOFFT_ERR_NULL;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return KOFFT_ERR_HIP;
    kofft_hip_ctx *ctx = new (std::nothrow) kofft_hip_ctx();
    if (!ctx) return KOFFT_ERR_ALLOC;
    ctx->device = device;
    // Route switches (each selects another implementation of the same transform; tests/test_gpu_knobs.py runs every one of them in
    // its non-default setting against the oracle).  The tuning knobs of rounds 1-3 that only ever confirmed the default are gone.
    if (const char *e = getenv("KOFFT_HIP_NO_PERSIST")) ctx->use_persist = !(e[0] == '1');
    if (const char *e = getenv("KOFFT_HIP_ISTFT_FUSED")) ctx->istft_fused = atoi(e) != 0;
    if (const char *e = getenv("KOFFT_HIP_BLUESTEIN_PERSIST")) ctx->blue_persist = atoi(e) != 0;
    if (const char *e = getenv("KOFFT_HIP_PERSIST_GRID_PCT")) ctx->persist_grid_pct = atoi(e);
    if (const char *e = getenv("KOFFT_HIP_BIG_THREE_MIN")) ctx->big_three_min = atoi(e);
    if (const char *e = getenv("KOFFT_HIP_SMALL32")) ctx->small32 = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_PERSIST")) ctx->big_persist = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_RFFT14_WIDE")) ctx->rfft14_wide = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_RFFT13_PERSIST")) ctx->rfft13_persist = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_PERSIST64")) ctx->persist64 = atoi(e);
    if (const char *e = getenv("KOFFT_HIP_PERSIST_SMALL")) ctx->persist_small = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_SPLIT")) ctx->use_split = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_REGFILE")) ctx->use_regfile = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_RFFT_REGFILE_EPI")) ctx->rfft_regfile_epi = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_HOST_PIPELINE")) ctx->host_pipeline = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_ZERO_COPY")) ctx->zero_copy = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_ND_TRANSPOSE")) ctx->nd_transpose = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BLUESTEIN_FUSED")) ctx->blue_fused = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BLUESTEIN_ONE")) ctx->blue_one_kernel = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_NARROW")) ctx->big_narrow = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_FIRST11")) ctx->big_first11 = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_ND_TWO_PASS")) ctx->nd_two_pass = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_ND_FUSED")) ctx->nd_fused = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_ROW_PAIRS")) ctx->big_row_pairs = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_BLOCKED")) ctx->big_blocked = !(e[0] == '0');
    if (const char *e = getenv("KOFFT_HIP_BIG_PROBE")) ctx->big_probe = atoi(e);
    if (const char *e = getenv("KOFFT_HIP_BIG_CHUNK_MB")) {
        const long mb = atol(e);
        if (mb > 0) ctx->big_chunk_bytes = (size_t)mb << 20;
    }
    if (const char *e = getenv("KOFFT_HIP_SCRATCH_CHUNK_MB")) (void)parse_scratch_chunk_mb(e, &ctx->scratch_chunk_bytes);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            ctx->num_cus = prop.multiProcessorCount;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return KOFFT_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    // the claim counters of the kClaim persistent kernels (fft_persist.hip.h): zero once, here; every launch leaves them at zero
    // (room for eight claim words, and the arrival word, each on a 128-byte line of its own)
    if (hipMalloc(reinterpret_cast<void **>(&ctx->persist_claim_counters), kofft::kPersistClaimBytes) != hipSuccess ||
        hipMemsetAsync(ctx->persist_claim_counters, 0, kofft::kPersistClaimBytes, ctx->own_stream) != hipSuccess) {
        if (ctx->persist_claim_counters) (void)hipFree(ctx->persist_claim_counters);
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return KOFFT_ERR_ALLOC;
    }
    *out = ctx;
    return KOFFT_OK;
}

int kofft_hip_destroy(kofft_hip_ctx *ctx)
{
    if (!ctx) return KOFFT_ERR_NULL;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &kv : ctx->tables) (void)hipFree(kv.second);
    spectral_drop(ctx);
    mel_drop(ctx);
    spec_drop(ctx);
    drop_buffers(ctx);
    if (ctx->persist_claim_counters) (void)hipFree(ctx->persist_claim_counters);
    if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return KOFFT_OK;
}

int kofft_hip_set_stream(kofft_hip_ctx *ctx, void *hip_stream)
{
    if (!ctx) return KOFFT_ERR_NULL;
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    if (next == ctx->stream) return KOFFT_OK;
    // The context's scratch (staging buffers, the large-n intermediate, the Bluestein work buffer) is ordered by stream
    // only: work still in flight on the old stream must finish before anything enqueued on the new one touches it.
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->order_event) KOFFT_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->order_event, hipEventDisableTiming));
    KOFFT_HIP_TRY(ctx, hipEventRecord(ctx->order_event, ctx->stream));
    KOFFT_HIP_TRY(ctx, hipStreamWaitEvent(next, ctx->order_event, 0));
    ctx->stream = next;
    return KOFFT_OK;
}

int kofft_hip_synchronize(kofft_hip_ctx *ctx)
{
    if (!ctx) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KOFFT_OK;
}

int kofft_hip_big_probe_info(kofft_hip_ctx *ctx, float *first_us, float *total_us, int cap, int *n, int *pick)
{
    if (!ctx || !n || !pick) return KOFFT_ERR_NULL;
    *n = ctx->big_probe_n;
    *pick = ctx->big_probe_pick;
    for (int i = 0; i < ctx->big_probe_n && i < cap; ++i) {
        if (first_us) first_us[i] = ctx->big_probe_first_us[i];
        if (total_us) total_us[i] = ctx->big_probe_total_us[i];
    }
    return KOFFT_OK;
}

int kofft_hip_release_scratch(kofft_hip_ctx *ctx)
{
    if (!ctx) return KOFFT_ERR_NULL;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    drop_buffers(ctx);
    spectral_drop(ctx);  // the chirp-Z tables (up to 4 x 128 MiB) and the Goertzel coefficient arrays: rebuilt by the next call that needs them
    mel_drop(ctx);       // the filterbank plans, likewise
    spec_drop(ctx);      // and the pixel ranges of the log-scaled spectrogram render
    ctx->big_probe_n = 0;
    ctx->big_probe_pick = -1;
    return KOFFT_OK;
}

int kofft_hip_twiddles_f32(size_t n, float *out)
{
    if (!out && n >= 2) return KOFFT_ERR_NULL;
    kofft_tables::twiddles_f32(n, out);
    return KOFFT_OK;
}
int kofft_hip_twiddles_f64(size_t n, double *out)
{
    if (!out && n >= 2) return KOFFT_ERR_NULL;
    kofft_tables::twiddles_f64(n, out);
    return KOFFT_OK;
}
int kofft_hip_rfft_table_f32(size_t m, float *out)
{
    if (!out && m) return KOFFT_ERR_NULL;
    kofft_tables::rfft_table_f32(m, out);
    return KOFFT_OK;
}
int kofft_hip_rfft_table_f64(size_t m, double *out)
{
    if (!out && m) return KOFFT_ERR_NULL;
    kofft_tables::rfft_table_f64(m, out);
    return KOFFT_OK;
}
int kofft_hip_dct2_table_f32(size_t n, float *cs)
{
    if (!cs && n) return KOFFT_ERR_NULL;
    kofft_tables::dct2_table_f32(n, cs);
    return KOFFT_OK;
}
static int direct_table(int family, int type, size_t n, float *c)
{
    if (type < 1 || type > 4) return KOFFT_ERR_INVALID_VALUE;
    if (n == 0) return KOFFT_OK;
    if (n > kofft::host::kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!c) return KOFFT_ERR_NULL;
    kofft_tables::direct_table_f32(family, type, n, n, c);
    return KOFFT_OK;
}
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
int kofft_hip_wavelet_taps_f32(int wavelet, int inverse, float *lo, float *hi)
{
    if (wavelet < 0 || wavelet > 4) return KOFFT_ERR_INVALID_VALUE;
    if (!lo || !hi) return KOFFT_ERR_NULL;
    wavelet_taps(wavelet, inverse != 0, lo, hi);
    return KOFFT_OK;
}
int kofft_hip_dwt_multi_lengths(size_t len, size_t levels, size_t *lens)
{
    if (levels > kWaveletMaxLevels) return KOFFT_ERR_UNSUPPORTED;
    if (!lens) return KOFFT_ERR_NULL;
    wavelet_lengths(len, levels, lens);
    return KOFFT_OK;
}
int kofft_hip_hann_f32(size_t len, float *out)
{
    if (!out && len) return KOFFT_ERR_NULL;
    kofft_tables::hann_f32(len, out);
    return KOFFT_OK;
}

int kofft_hip_fft_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch, int inverse)
{
    return fft_host<float>(ctx, data, n, batch, inverse);
}
int kofft_hip_fft_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch, int inverse)
{
    return fft_host<double>(ctx, data, n, batch, inverse);
}
int kofft_hip_fft_c32_dev(kofft_hip_ctx *ctx, float *d_data, size_t n, size_t batch, int inverse)
{
    return fft_dev<float>(ctx, d_data, d_data, n, batch, inverse);
}
int kofft_hip_fft_c64_dev(kofft_hip_ctx *ctx, double *d_data, size_t n, size_t batch, int inverse)
{
    return fft_dev<double>(ctx, d_data, d_data, n, batch, inverse);
}
int kofft_hip_fft_c32_dev_oop(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch,
                              int inverse)
{
    return fft_dev<float>(ctx, d_in, d_out, n, batch, inverse);
}
int kofft_hip_fft_c64_dev_oop(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch,
                              int inverse)
{
    return fft_dev<double>(ctx, d_in, d_out, n, batch, inverse);
}
int kofft_hip_fft_split_c32(kofft_hip_ctx *ctx, float *re, float *im, size_t n, size_t batch, int inverse)
{
    return planar_host<float>(ctx, re, im, n, batch, inverse);
}
int kofft_hip_fft_split_c64(kofft_hip_ctx *ctx, double *re, double *im, size_t n, size_t batch, int inverse)
{
    return planar_host<double>(ctx, re, im, n, batch, inverse);
}
int kofft_hip_dev_fft_split_c32(kofft_hip_ctx *ctx, const float *d_re_in, const float *d_im_in, float *d_re_out, float *d_im_out, size_t n,
                                size_t batch, int inverse)
{
    return planar_dev<float>(ctx, d_re_in, d_im_in, d_re_out, d_im_out, n, batch, inverse);
}
int kofft_hip_dev_fft_split_c64(kofft_hip_ctx *ctx, const double *d_re_in, const double *d_im_in, double *d_re_out, double *d_im_out, size_t n,
                                size_t batch, int inverse)
{
    return planar_dev<double>(ctx, d_re_in, d_im_in, d_re_out, d_im_out, n, batch, inverse);
}
int kofft_hip_set_split_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->planar_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_fft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch) { return fft_radix4_host<float>(ctx, data, n, batch, 0); }
int kofft_hip_fft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch) { return fft_radix4_host<double>(ctx, data, n, batch, 0); }
int kofft_hip_fft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<float>(ctx, d_in, d_out, n, batch, 0);
}
int kofft_hip_fft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<double>(ctx, d_in, d_out, n, batch, 0);
}
int kofft_hip_ifft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch) { return fft_radix4_host<float>(ctx, data, n, batch, 1); }
int kofft_hip_ifft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch) { return fft_radix4_host<double>(ctx, data, n, batch, 1); }
int kofft_hip_ifft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<float>(ctx, d_in, d_out, n, batch, 1);
}
int kofft_hip_ifft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch)
{
    return fft_radix4_dev<double>(ctx, d_in, d_out, n, batch, 1);
}
int kofft_hip_fft_c32_strided(kofft_hip_ctx *ctx, float *data, size_t data_len, size_t stride, size_t n,
                              int inverse)
{
    return fft_strided_host<float>(ctx, data, data_len, stride, n, inverse);
}
int kofft_hip_fft_c64_strided(kofft_hip_ctx *ctx, double *data, size_t data_len, size_t stride, size_t n,
                              int inverse)
{
    return fft_strided_host<double>(ctx, data, data_len, stride, n, inverse);
}

int kofft_hip_rfft_f32(kofft_hip_ctx *ctx, const float *in, float *out, const float *window, size_t n,
                       size_t batch)
{
    return rfft_host<float>(ctx, in, out, window, n, batch);
}
int kofft_hip_rfft_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *d_window, size_t n,
                           size_t batch)
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
int kofft_hip_set_dct_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->dct_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_dct2_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    return dct2_host(ctx, in, out, n, batch);
}
int kofft_hip_dct2_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return dct2_dev(ctx, d_in, d_out, n, batch);
}
int kofft_hip_set_hilbert_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->hilbert_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_hilbert_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    return hilbert_host(ctx, in, out, n, batch);
}
int kofft_hip_hilbert_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return hilbert_dev(ctx, d_in, d_out, n, batch);
}
int kofft_hip_set_cepstrum_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->cepstrum_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_cepstrum_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    return cepstrum_host(ctx, in, out, n, batch);
}
int kofft_hip_cepstrum_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return cepstrum_dev(ctx, d_in, d_out, n, batch);
}
int kofft_hip_set_convolve_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->convolve_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_convolve_block(size_t nx, size_t nh, size_t *block)
{
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nx > (SIZE_MAX >> 2) || nh > (SIZE_MAX >> 2)) return KOFFT_ERR_UNSUPPORTED;
    if (!block) return KOFFT_ERR_NULL;
    *block = convolve_default_block(nx, nh);
    return KOFFT_OK;
}
int kofft_hip_convolve_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh, size_t block,
                           unsigned flags, float *out, size_t out_first, size_t out_len)
{
    return convolve_host(ctx, x, rows, nx, h, filters, nh, block, flags, out, out_first, out_len);
}
int kofft_hip_dev_convolve_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                               size_t block, unsigned flags, float *d_out, size_t out_first, size_t out_len)
{
    return convolve_dev(ctx, d_x, rows, nx, d_h, filters, nh, block, flags, d_out, out_first, out_len);
}
int kofft_hip_set_convolve_bank_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->convolve_bank_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_convolve_bank_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh,
                                size_t block, unsigned flags, void *out, size_t out_first, size_t out_len)
{
    return convolve_bank_host(ctx, x, rows, nx, h, filters, nh, block, flags, out, out_first, out_len);
}
int kofft_hip_dev_convolve_bank_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                                    size_t block, unsigned flags, void *d_out, size_t out_first, size_t out_len)
{
    return convolve_bank_dev(ctx, d_x, rows, nx, d_h, filters, nh, block, flags, d_out, out_first, out_len);
}
// ---- polyphase resampling of rows (k_resample_f32.hip) -----------------------------------------------------------
// nx samples per row go up, out_len values come down; the one filter is the side input, uploaded once
int kofft_hip_resample_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t nh, size_t up, size_t down,
                           size_t t0, float *out, size_t out_len)
{
    const int rc = resample_check(rows, nx, nh, up, down, t0, out_len, x, h, out, ctx);
    if (rc || rows == 0 || out_len == 0) return rc;
    return rows_host<float>(ctx, x, out, rows, nx, out_len, h, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return resample_dev(ctx, d_in, nr, nx, d_h, nh, up, down, t0, d_out, out_len);
                            });
}
int kofft_hip_dev_resample_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t nh, size_t up,
                               size_t down, size_t t0, float *d_out, size_t out_len)
{
    return resample_dev(ctx, d_x, rows, nx, d_h, nh, up, down, t0, d_out, out_len);
}
int kofft_hip_set_resample_tiled(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (on < 0 || on > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->resample_tiled = on;
    return KOFFT_OK;
}
int kofft_hip_resample_route(size_t nh, size_t up, size_t down, int *route)
{
    if (!route) return KOFFT_ERR_NULL;
    if (nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (up == 0 || down == 0) return KOFFT_ERR_INVALID_VALUE;
    *route = resample_route(nh, up, down);
    return KOFFT_OK;
}
int kofft_hip_resample_taps_f32(size_t up, size_t down, size_t zeros, double beta, float *taps, size_t *nh)
{
    return resample_taps(up, down, zeros, beta, taps, nh);
}
// ---- IIR filtering of rows by a cascade of biquads (k_sosfilt_f32.hip) -------------------------------------------
// up to four row arrays: x up, out down, zi up, zf down (an absent state is an empty array and reaches the device as null); the
// coefficients are the side input, uploaded once
int kofft_hip_sosfilt_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                          float *zf, unsigned flags, float *out)
{
    const int rc = sosfilt_check(rows, nx, sections, flags, x, sos, zi, zf, out, ctx, true);
    if (rc || rows == 0 || nx == 0) return rc;
    const HostArray<float> a[4] = {{x, nullptr, nx}, {nullptr, out, nx}, {zi, nullptr, zi ? 2 * sections : 0}, {nullptr, zf, zf ? 2 * sections : 0}};
    return rows_host_n<float>(ctx, rows, 4, a, sos, 6 * sections, true, true, [&](float *const *d, const float *d_sos, size_t nr) {
        return sosfilt_dev(ctx, d[0], nr, nx, d_sos, sections, zi ? d[2] : nullptr, zf ? d[3] : nullptr, flags, d[1]);
    });
}
int kofft_hip_dev_sosfilt_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                              const float *d_zi, float *d_zf, unsigned flags, float *d_out)
{
    return sosfilt_dev(ctx, d_x, rows, nx, d_sos, sections, d_zi, d_zf, flags, d_out);
}
// ---- the same cascade as a scan along time (k_sosfilt_f32.hip): the same staging, rows are independent -------------
int kofft_hip_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                               float *zf, size_t chunk, unsigned flags, float *out)
{
    const int rc = sosfilt_check(rows, nx, sections, flags, x, sos, zi, zf, out, ctx, true, &chunk);
    if (rc || rows == 0 || nx == 0) return rc;
    const HostArray<float> a[4] = {{x, nullptr, nx}, {nullptr, out, nx}, {zi, nullptr, zi ? 2 * sections : 0}, {nullptr, zf, zf ? 2 * sections : 0}};
    return rows_host_n<float>(ctx, rows, 4, a, sos, 6 * sections, true, true, [&](float *const *d, const float *d_sos, size_t nr) {
        return sosfilt_scan_dev(ctx, d[0], nr, nx, d_sos, sections, zi ? d[2] : nullptr, zf ? d[3] : nullptr, chunk, flags, d[1]);
    });
}
int kofft_hip_dev_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                                   const float *d_zi, float *d_zf, size_t chunk, unsigned flags, float *d_out)
{
    return sosfilt_scan_dev(ctx, d_x, rows, nx, d_sos, sections, d_zi, d_zf, chunk, flags, d_out);
}
int kofft_hip_sosfilt_scan_chunk(size_t rows, size_t nx, size_t sections, size_t *chunk)
{
    if (!chunk) return KOFFT_ERR_NULL;
    *chunk = (size_t)sos_scan_chunk_rule(rows, nx, sections);
    return KOFFT_OK;
}
int kofft_hip_sosfilt_route(size_t rows, int *route)
{
    if (!route) return KOFFT_ERR_NULL;
    *route = sos_route(rows);
    return KOFFT_OK;
}
int kofft_hip_set_sosfilt_tiled(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (on < 0 || on > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->sosfilt_tiled = on;
    return KOFFT_OK;
}
int kofft_hip_set_mfcc_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (on < 0 || on > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->mfcc_fused = on;
    return KOFFT_OK;
}
int kofft_hip_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *mags, float *energies, size_t n_fft, size_t rows, const uint64_t *bins,
                                 size_t num_mel)
{
    return mel_host(ctx, false, mags, energies, n_fft, rows, bins, num_mel, 0);
}
int kofft_hip_dev_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_energies, size_t n_fft, size_t rows,
                                     const uint64_t *bins, size_t num_mel)
{
    return mel_filterbank_dev(ctx, d_mags, d_energies, n_fft, rows, bins, num_mel);
}
int kofft_hip_mfcc_f32(kofft_hip_ctx *ctx, const float *mags, float *coeffs, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
                       size_t num_coeffs)
{
    return mel_host(ctx, true, mags, coeffs, n_fft, rows, bins, num_mel, num_coeffs);
}
int kofft_hip_dev_mfcc_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const uint64_t *bins,
                           size_t num_mel, size_t num_coeffs)
{
    return mfcc_dev(ctx, d_mags, d_coeffs, n_fft, rows, bins, num_mel, num_coeffs);
}
int kofft_hip_mel_bins_f32(float sample_rate, size_t n_fft, size_t num_filters, uint64_t *bins)
{
    if (num_filters > kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!bins) return KOFFT_ERR_NULL;
    kofft_tables::mel_bins_f32(sample_rate, n_fft, num_filters, bins);
    return KOFFT_OK;
}
int kofft_hip_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float floor_db, float *out)
{
    return spec_db_host(ctx, 0, mags, count, max_mag, floor_db, out);
}
int kofft_hip_dev_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float floor_db,
                                      float *d_out)
{
    return spec_db_dev(ctx, 0, d_mags, count, d_max_mag, floor_db, d_out);
}
int kofft_hip_db_scale_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float dynamic_range, float *out)
{
    return spec_db_host(ctx, 1, mags, count, max_mag, dynamic_range, out);
}
int kofft_hip_dev_db_scale_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float dynamic_range,
                               float *d_out)
{
    return spec_db_dev(ctx, 1, d_mags, count, d_max_mag, dynamic_range, d_out);
}
int kofft_hip_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *mags, size_t frames, size_t bins, const float *max_mag, int mode,
                                     float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin, void *out)
{
    return spec_render_host(ctx, mags, frames, bins, max_mag, mode, level, cmap, depth, scale, layout, pix_of_bin, out);
}
int kofft_hip_dev_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t frames, size_t bins, const float *d_max_mag,
                                         int mode, float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin,
                                         void *d_out)
{
    return spec_render_dev(ctx, d_mags, frames, bins, d_max_mag, mode, level, cmap, depth, scale, layout, pix_of_bin, d_out);
}
int kofft_hip_set_spectrogram_transpose(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->spec_transpose = on != 0;
    return KOFFT_OK;
}
int kofft_hip_log_bin_map(size_t bins, uint32_t *pix_of_bin)
{
    if (bins == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (bins > kSpecMaxBins) return KOFFT_ERR_UNSUPPORTED;
    if (!pix_of_bin) return KOFFT_ERR_NULL;
    kofft_tables::log_bin_map(bins, pix_of_bin);
    return KOFFT_OK;
}
int kofft_hip_map_color_u8(float t, int cmap, unsigned char *rgb) { return spec_map_color_u8(t, cmap, rgb); }
int kofft_hip_set_direct_tiled(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->direct_tiled = on != 0;
    return KOFFT_OK;
}
int kofft_hip_set_persist_claim_pct(kofft_hip_ctx *ctx, int pct)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (pct > 100) return KOFFT_ERR_INVALID_VALUE;
    ctx->persist_claim_pct = pct < 0 ? -1 : pct;
    return KOFFT_OK;
}
int kofft_hip_persist_claim_debug(kofft_hip_ctx *ctx, unsigned out[9])
{
    if (!ctx || !out) return KOFFT_ERR_NULL;
    if (!ctx->persist_claim_counters) return KOFFT_ERR_ALLOC;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    KOFFT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (unsigned s = 0; s <= kofft::kPersistClaimMaxShards; ++s)
        KOFFT_HIP_TRY(ctx, hipMemcpy(out + s, ctx->persist_claim_counters + s * kofft::kPersistClaimLine, sizeof(unsigned), hipMemcpyDeviceToHost));
    return KOFFT_OK;
}
int kofft_hip_set_persist_walk(kofft_hip_ctx *ctx, int mode)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (mode < -1 || mode > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->persist_walk_mode = mode;
    return KOFFT_OK;
}
int kofft_hip_set_persist_keep_bytes(kofft_hip_ctx *ctx, size_t bytes)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->persist_keep_bytes = bytes;
    return KOFFT_OK;
}
int kofft_hip_persist_walk_debug(kofft_hip_ctx *ctx, unsigned long long out[4])
{
    if (!ctx || !out) return KOFFT_ERR_NULL;
    out[0] = ctx->persist_walk_launches;  // host-side state only: no synchronisation
    out[1] = ctx->persist_walk_plan_last.mirror ? 1u : 0u;
    out[2] = ctx->persist_walk_plan_last.keep_from;
    out[3] = ctx->persist_walk_batch_last;
    return KOFFT_OK;
}
int kofft_hip_set_wavelet_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (on < 0 || on > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->wavelet_fused = on;
    return KOFFT_OK;
}
int kofft_hip_dwt_f32(kofft_hip_ctx *ctx, int wavelet, const float *in, float *approx, float *detail, size_t len, size_t batch)
{
    return dwt_host(ctx, wavelet, in, approx, detail, len, batch);
}
int kofft_hip_dwt_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_in, float *d_approx, float *d_detail, size_t len, size_t batch)
{
    return dwt_dev(ctx, wavelet, d_in, d_approx, d_detail, len, batch);
}
int kofft_hip_idwt_f32(kofft_hip_ctx *ctx, int wavelet, const float *approx, const float *detail, float *out, size_t n, size_t batch)
{
    return idwt_host(ctx, wavelet, approx, detail, out, n, batch);
}
int kofft_hip_idwt_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_approx, const float *d_detail, float *d_out, size_t n, size_t batch)
{
    return idwt_dev(ctx, wavelet, d_approx, d_detail, d_out, n, batch);
}
int kofft_hip_dwt_multi_f32(kofft_hip_ctx *ctx, int wavelet, const float *in, float *approx, float *details, size_t len, size_t batch,
                            size_t levels)
{
    return dwt_multi_host(ctx, wavelet, in, approx, details, len, batch, levels);
}
int kofft_hip_dwt_multi_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_in, float *d_approx, float *d_details, size_t len,
                                size_t batch, size_t levels)
{
    return dwt_multi_dev(ctx, wavelet, d_in, d_approx, d_details, len, batch, levels);
}
int kofft_hip_idwt_multi_f32(kofft_hip_ctx *ctx, int wavelet, const float *approx, const float *details, const size_t *detail_lens,
                             float *out, size_t n, size_t batch, size_t levels)
{
    return idwt_multi_host(ctx, wavelet, approx, details, detail_lens, out, n, batch, levels);
}
int kofft_hip_idwt_multi_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_approx, const float *d_details, const size_t *detail_lens,
                                 float *d_out, size_t n, size_t batch, size_t levels)
{
    return idwt_multi_dev(ctx, wavelet, d_approx, d_details, detail_lens, d_out, n, batch, levels);
}
int kofft_hip_czt_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t m, float wr, float wi, float ar, float ai, size_t batch)
{
    return czt_host(ctx, in, out, n, m, wr, wi, ar, ai, batch);
}
int kofft_hip_dev_czt_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t m, float wr, float wi, float ar, float ai,
                          size_t batch)
{
    return czt_dev(ctx, d_in, d_out, n, m, wr, wi, ar, ai, batch);
}
int kofft_hip_goertzel_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch, float sample_rate,
                           const float *target_freqs, size_t nfreq)
{
    return goertzel_host(ctx, in, out, n, batch, sample_rate, target_freqs, nfreq);
}
int kofft_hip_dev_goertzel_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch, float sample_rate,
                               const float *target_freqs, size_t nfreq)
{
    return goertzel_dev(ctx, d_in, d_out, n, batch, sample_rate, target_freqs, nfreq);
}
int kofft_hip_set_czt_route(kofft_hip_ctx *ctx, int mode)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (mode < 0 || mode > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->czt_route = mode;
    return KOFFT_OK;
}
int kofft_hip_czt_table_f32(size_t n, size_t m, float wr, float wi, float ar, float ai, float *C)
{
    if (n == 0 || m == 0) return KOFFT_OK;
    if (n > kCztMax || m > kCztMax) return KOFFT_ERR_UNSUPPORTED;
    if (!C) return KOFFT_ERR_NULL;
    kofft_tables::czt_table_f32(n, m, wr, wi, ar, ai, 2 * m, C);
    return KOFFT_OK;
}
int kofft_hip_goertzel_coeff_f32(size_t n, float sample_rate, const float *target_freqs, size_t nfreq, float *coeff)
{
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (sample_rate <= 0.0f) return KOFFT_ERR_INVALID_VALUE;
    if (nfreq == 0) return KOFFT_OK;
    if (n > kGoertzelMaxLen || nfreq > kGoertzelMaxFreqs) return KOFFT_ERR_UNSUPPORTED;
    if (!target_freqs || !coeff) return KOFFT_ERR_NULL;
    kofft_tables::goertzel_coeff_f32(n, sample_rate, target_freqs, nfreq, coeff);
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
int kofft_hip_dht_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch) { return dht_host(ctx, in, out, n, batch); }
int kofft_hip_dev_dht_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return dht_dev(ctx, d_in, d_out, n, batch);
}
int kofft_hip_set_dht_table_device(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->dht_table_device = on != 0;
    return KOFFT_OK;
}
int kofft_hip_dht_table_f32(size_t n, float *H)
{
    if (n == 0) return KOFFT_OK;
    if (n > kofft::host::kDirectMaxN) return KOFFT_ERR_UNSUPPORTED;
    if (!H) return KOFFT_ERR_NULL;
    kofft_tables::dht_table_f32(n, n, H);
    return KOFFT_OK;
}
int kofft_hip_libm_trigf(const float *x, size_t count, float *cos_out, float *sin_out)
{
    if (count == 0) return KOFFT_OK;
    if (!x || !cos_out || !sin_out) return KOFFT_ERR_NULL;
    return kofft_tables::libm_trigf(x, count, cos_out, sin_out) ? KOFFT_OK : KOFFT_ERR_UNSUPPORTED;
}
int kofft_hip_window_f32(int kind, size_t len, float param, float *out)
{
    if (kind < 0 || kind >= kofft_tables::kWindowKinds) return KOFFT_ERR_INVALID_VALUE;
    if (len == 0) return kind == KOFFT_WINDOW_KAISER ? KOFFT_ERR_EMPTY_INPUT : KOFFT_OK;
    if (!out) return KOFFT_ERR_NULL;
    kofft_tables::window_f32(kind, len, param, out);
    return KOFFT_OK;
}
int kofft_hip_rfft_f64(kofft_hip_ctx *ctx, const double *in, double *out, const double *window, size_t n,
                       size_t batch)
{
    return rfft_host<double>(ctx, in, out, window, n, batch);
}
int kofft_hip_rfft_f64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, const double *d_window,
                           size_t n, size_t batch)
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

int kofft_hip_stft_f32(kofft_hip_ctx *ctx, const float *signal, size_t len, const float *window, size_t win_len,
                       size_t hop, float *out, size_t frames)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;               // stft.rs:83
    const size_t required = len / hop + (len % hop != 0);                  // stft.rs:86
    if (frames < required) return KOFFT_ERR_MISMATCHED_LENGTHS;    // stft.rs:87
    return stft_host(ctx, signal, len, window, win_len, 0, hop, out, frames);
}

int kofft_hip_stft_parallel_f32(kofft_hip_ctx *ctx, const float *signal, size_t len, const float *window,
                                size_t win_len, size_t hop, float *out, size_t frames)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;  // stft.rs:242 -- the only check parallel() makes
    return stft_host(ctx, signal, len, window, win_len, 0, hop, out, frames);
}

int kofft_hip_stft_frame_f32(kofft_hip_ctx *ctx, const float *signal, size_t len, const float *window,
                             size_t win_len, size_t start, float *frame_out)
{
    return stft_host(ctx, signal, len, window, win_len, start, 1, frame_out, 1);
}

int kofft_hip_stft_f32_dev(kofft_hip_ctx *ctx, const float *d_signal, size_t len, const float *d_window,
                           size_t win_len, size_t hop, float *d_out, size_t first_frame, size_t count)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;  // stft.rs:83 / 242
    return stft_dev(ctx, d_signal, len, d_window, win_len, first_frame * hop, hop, d_out, count);
}

int kofft_hip_istft_f32_dev(kofft_hip_ctx *ctx, float *d_frames, size_t frames, const float *d_window, size_t win_len,
                            size_t hop, float *d_output, size_t out_len, float *d_scratch, size_t scratch_len)
{
    return istft_dev(ctx, d_frames, frames, d_window, win_len, hop, d_output, out_len, d_scratch, scratch_len);
}

int kofft_hip_istft_f32(kofft_hip_ctx *ctx, float *frames_data, size_t frames, const float *window, size_t win_len,
                        size_t hop, float *output, size_t out_len, float *scratch, size_t scratch_len)
{
    return istft_host(ctx, frames_data, frames, window, win_len, hop, output, out_len, scratch, scratch_len, 1, 0);
}

int kofft_hip_istft_parallel_f32(kofft_hip_ctx *ctx, const float *frames_data, size_t frames, const float *window,
                                 size_t win_len, size_t hop, float *output, size_t out_len)
{
    // inverse_parallel clones each frame (stft.rs:310): the caller's frames are left untouched
    return istft_host(ctx, const_cast<float *>(frames_data), frames, window, win_len, hop, output, out_len, nullptr, out_len, 2, 0);
}

int kofft_hip_istft_frame_f32(kofft_hip_ctx *ctx, float *frame, const float *window, size_t win_len, size_t start,
                              float *output, size_t out_len)
{
    // inverse_frame (stft.rs:384-399): ifft(frame) in place, output[start + i] += frame[i].re * window[i], no normalisation
    return istft_host(ctx, frame, 1, window, win_len, win_len ? win_len : 1, output, out_len, nullptr, out_len, 0, start);
}

int kofft_hip_stft_magnitudes_f32_dev(kofft_hip_ctx *ctx, const float *d_samples, size_t len, size_t win_len, size_t hop,
                                      float *d_mags, size_t frames, float *d_max)
{
    return stft_mag_dev(ctx, d_samples, len, win_len, hop, d_mags, frames, d_max);
}

int kofft_hip_stft_magnitudes_f32(kofft_hip_ctx *ctx, const float *samples, size_t len, size_t win_len, size_t hop,
                                  float *mags, size_t frames, float *max_mag)
{
    if (hop == 0) return KOFFT_ERR_INVALID_HOP_SIZE;
    if (frames < len / hop + (len % hop != 0)) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (frames > 0 && win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (frames > 0 && !complex_len_ok(win_len)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !max_mag || (frames && (!mags || (!samples && len)))) return KOFFT_ERR_NULL;
    // never zero-copy: the maximum is an atomicMax target and stays in device memory
    const HostArray<float> a[3] = {{samples, nullptr, len}, {nullptr, mags, frames * (win_len / 2)}, {nullptr, max_mag, 1}};
    return stage_host<float>(ctx, 1, 3, a, nullptr, 0, false, false, [&](float *const *d, const float *, size_t) {
        return stft_mag_dev(ctx, d[0], len, win_len, hop, d[1], frames, d[2]);
    });
}

// ---- STFT, stft_magnitudes and ISTFT over rows of signals (k_stft_rows.hip) --------------------------------------
// Host rows `row_stride` apart are packed (stride len) before they travel: the gaps are not the call's to read.
static const float *pack_rows(const float *signal, size_t rows, size_t len, size_t row_stride, std::vector<float> &packed)
{
    if (len == 0 || rows == 1 || row_stride == len) return signal;
    packed.resize(rows * len);
    for (size_t r = 0; r < rows; ++r) std::copy_n(signal + r * row_stride, len, packed.data() + r * len);
    return packed.data();
}

int kofft_hip_dev_stft_rows_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                const float *d_window, size_t win_len, size_t hop, float *d_out, size_t frames)
{
    return stft_rows_dev(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, d_out, frames);
}

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
                                return stft_rows_dev(ctx, d_in, nb, len, len, d_win, win_len, hop, d_out, frames);
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
    // never zero-copy: the maxima are atomicMax targets and stay in device memory, as in the single-signal form above
    const HostArray<float> a[3] = {{src, nullptr, len}, {nullptr, mags, frames * (win_len / 2)}, {nullptr, max_mag, 1}};
    return rows_host_n<float>(ctx, rows, 3, a, nullptr, 0, false, true, [&](float *const *d, const float *, size_t nb) {
        return stft_mag_rows_dev(ctx, d[0], nb, len, len, win_len, hop, d[1], frames, d[2]);
    });
}

// ---- rows of audio to mel energies / MFCCs (k_frontend_f32.hip) --------------------------------------------------
// The signal goes up, the energies or coefficients come down (whole rows per chunk of the pipeline); the magnitudes stay on the device.
static int frontend_host(kofft_hip_ctx *ctx, bool mfcc, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                         size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs, float *out)
{
    const int crc = frontend_check(mfcc, false, signal, window, out, rows, len, row_stride, win_len, hop, frames, bins, num_mel, num_coeffs, ctx);
    if (crc || rows == 0 || frames == 0 || num_mel == 0 || (mfcc && num_coeffs == 0)) return crc;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, len, frames * (mfcc ? num_coeffs : num_mel), window, window ? win_len : 0, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return frontend_dev(ctx, mfcc, d_in, nb, len, len, d_win, win_len, hop, frames, bins, num_mel, num_coeffs, d_out);
                            });
}

int kofft_hip_stft_mel_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                                size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, float *energies)
{
    return frontend_host(ctx, false, signal, rows, len, row_stride, window, win_len, hop, frames, bins, num_mel, 0, energies);
}

int kofft_hip_dev_stft_mel_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                    const float *d_window, size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel,
                                    float *d_energies)
{
    return frontend_dev(ctx, false, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins, num_mel, 0, d_energies);
}

int kofft_hip_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                                 size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs,
                                 float *coeffs)
{
    return frontend_host(ctx, true, signal, rows, len, row_stride, window, win_len, hop, frames, bins, num_mel, num_coeffs, coeffs);
}

int kofft_hip_dev_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                     const float *d_window, size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel,
                                     size_t num_coeffs, float *d_coeffs)
{
    return frontend_dev(ctx, true, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins, num_mel, num_coeffs, d_coeffs);
}

// ---- rows of audio to spectrogram pictures (k_picture_f32.hip) ---------------------------------------------------
// The signal (and mode 2's maxima) go up, the pictures and the maxima come down, all as bytes, whole rows per chunk of the pipeline: a
// row's running maximum never crosses a chunk of the pipeline.  Never zero-copy: the maxima are atomicMax targets and stay in device memory.
int kofft_hip_stft_picture_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                               size_t win_len, size_t hop, size_t frames, int max_mode, const float *max_in, float *max_out, int mode,
                               float level, int cmap, int depth, int channels, int scale, int layout, const uint32_t *pix_of_bin, void *out)
{
    bool empty = false;
    const int crc = picture_check(false, signal, rows, len, row_stride, window, win_len, hop, frames, max_mode, max_in, max_out, mode, cmap,
                                  depth, channels, scale, layout, pix_of_bin, out, ctx, &empty);
    if (crc || rows == 0 || frames == 0) return crc;
    if (empty) {
        if (max_mode == 2 && !max_in) return KOFFT_ERR_NULL;
        for (size_t r = 0; max_out && r < rows; ++r) max_out[r] = max_mode == 2 ? max_in[r] : (max_mode == 1 ? 1e-12f : 0.0f);
        return KOFFT_OK;
    }
    typedef unsigned char byte;
    std::vector<float> packed;
    const float *src = pack_rows(signal, rows, len, row_stride, packed);
    const size_t px = channels == 4 ? 4 : (depth == 16 ? 6 : 3);
    const HostArray<byte> a[4] = {{reinterpret_cast<const byte *>(src), nullptr, len * sizeof(float)},
                                  {nullptr, static_cast<byte *>(out), frames * (win_len / 2) * px},
                                  {max_mode == 2 ? reinterpret_cast<const byte *>(max_in) : nullptr, nullptr, sizeof(float)},
                                  {nullptr, reinterpret_cast<byte *>(max_out), sizeof(float)}};
    return rows_host_n<byte>(ctx, rows, 4, a, reinterpret_cast<const byte *>(window), window ? win_len * sizeof(float) : 0, false, true,
                             [&](byte *const *d, const byte *d_win, size_t nb) {
                                 return picture_dev(ctx, reinterpret_cast<const float *>(d[0]), nb, len, len, reinterpret_cast<const float *>(d_win),
                                                    win_len, hop, frames, max_mode, max_mode == 2 ? reinterpret_cast<const float *>(d[2]) : nullptr,
                                                    max_out ? reinterpret_cast<float *>(d[3]) : nullptr, mode, level, cmap, depth, channels, scale,
                                                    layout, pix_of_bin, d[1]);
                             });
}

int kofft_hip_dev_stft_picture_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                   const float *d_window, size_t win_len, size_t hop, size_t frames, int max_mode, const float *d_max_in,
                                   float *d_max_out, int mode, float level, int cmap, int depth, int channels, int scale, int layout,
                                   const uint32_t *pix_of_bin, void *d_out)
{
    return picture_dev(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, max_mode, d_max_in, d_max_out, mode, level, cmap,
                       depth, channels, scale, layout, pix_of_bin, d_out);
}

int kofft_hip_set_frontend_fused(kofft_hip_ctx *ctx, int mode)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (mode < 0 || mode > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->frontend_fused = mode;
    return KOFFT_OK;
}

// ---- fast DCT-IV of rows, MDCT of rows of signals and IMDCT (k_mdct_f32.hip) ----------------------------------------
// Whole rows per chunk of the host pipeline; the window is the side input, uploaded once.
int kofft_hip_dct4_table_f32(size_t n, float *out)
{
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n & 1) return KOFFT_ERR_INVALID_VALUE;
    if (!out) return KOFFT_ERR_NULL;
    kofft_tables::dct4_table_f32(n, out);
    return KOFFT_OK;
}
int kofft_hip_set_mdct_fused(kofft_hip_ctx *ctx, int on)
{
    if (!ctx) return KOFFT_ERR_NULL;
    ctx->mdct_fused = on != 0;
    return KOFFT_OK;
}
int kofft_hip_dev_dct4_fast_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    return dct4_fast_dev(ctx, d_in, d_out, n, batch);
}
int kofft_hip_dct4_fast_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = dct4_fast_check(n, batch, in, out, ctx);
    if (crc || batch == 0) return crc;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true,
                            [&](float *d_in, float *d_out, const float *, size_t nb) { return dct4_fast_dev(ctx, d_in, d_out, n, nb); });
}
int kofft_hip_dev_mdct_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, size_t row_stride, const float *d_window, size_t n,
                           size_t lead, float *d_out, size_t frames)
{
    return mdct_dev(ctx, d_x, rows, nx, row_stride, d_window, n, lead, d_out, frames);
}
int kofft_hip_mdct_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, size_t row_stride, const float *window, size_t n, size_t lead,
                       float *out, size_t frames)
{
    const int crc = mdct_check(rows, nx, row_stride, n, lead, frames, x, window, out, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    std::vector<float> packed;
    const float *src = pack_rows(x, rows, nx, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, nx, frames * n, window, 2 * n, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return mdct_dev(ctx, d_in, nb, nx, nx, d_win, n, lead, d_out, frames);
                            });
}
int kofft_hip_dev_imdct_f32(kofft_hip_ctx *ctx, const float *d_coef, size_t rows, size_t frames, const float *d_window, size_t n, float scale,
                            float *d_out, size_t out_first, size_t out_len)
{
    return imdct_dev(ctx, d_coef, rows, frames, d_window, n, scale, d_out, out_first, out_len);
}
int kofft_hip_imdct_f32(kofft_hip_ctx *ctx, const float *coef, size_t rows, size_t frames, const float *window, size_t n, float scale, float *out,
                        size_t out_first, size_t out_len)
{
    const int crc = imdct_check(rows, frames, n, out_first, out_len, coef, window, out, ctx);
    if (crc || rows == 0 || frames == 0 || out_len == 0) return crc;
    return rows_host<float>(ctx, coef, out, rows, frames * n, out_len, window, 2 * n, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return imdct_dev(ctx, d_in, nb, frames, d_win, n, scale, d_out, out_first, out_len);
                            });
}

// ---- Welch power spectra and cross spectra of rows (k_welch_f32.hip) ----------------------------------------------
// The signals go up, rows * K values come down (whole rows per chunk of the pipeline); no frame leaves the device.
static int welch_host(kofft_hip_ctx *ctx, bool csd, const float *x, const float *y, size_t rows, size_t len, size_t row_stride,
                      const float *window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *out)
{
    const int crc = welch_check(csd, x, y, window, out, rows, len, row_stride, win_len, hop, frames, flags, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    const size_t out_row = (win_len / 2 + 1) * (csd ? 2 : 1);
    std::vector<float> packed_x, packed_y;
    const float *sx = pack_rows(x, rows, len, row_stride, packed_x);
    if (!csd)
        return rows_host<float>(ctx, sx, out, rows, len, out_row, window, window ? win_len : 0, true, true,
                                [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                    return welch_dev(ctx, false, d_in, nullptr, nb, len, len, d_win, win_len, hop, frames, scale, flags, d_out);
                                });
    const float *sy = pack_rows(y, rows, len, row_stride, packed_y);
    const HostArray<float> a[3] = {{sx, nullptr, len}, {sy, nullptr, len}, {nullptr, out, out_row}};
    return rows_host_n<float>(ctx, rows, 3, a, window, window ? win_len : 0, true, true, [&](float *const *d, const float *d_win, size_t nb) {
        return welch_dev(ctx, true, d[0], d[1], nb, len, len, d_win, win_len, hop, frames, scale, flags, d[2]);
    });
}

int kofft_hip_welch_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                        size_t win_len, size_t hop, size_t frames, float scale, int flags, float *psd)
{
    return welch_host(ctx, false, signal, nullptr, rows, len, row_stride, window, win_len, hop, frames, scale, flags, psd);
}

int kofft_hip_dev_welch_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                            size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_psd)
{
    return welch_dev(ctx, false, d_signal, nullptr, rows, len, row_stride, d_window, win_len, hop, frames, scale, flags, d_psd);
}

int kofft_hip_csd_f32(kofft_hip_ctx *ctx, const float *x, const float *y, size_t rows, size_t len, size_t row_stride, const float *window,
                      size_t win_len, size_t hop, size_t frames, float scale, int flags, float *pxy)
{
    return welch_host(ctx, true, x, y, rows, len, row_stride, window, win_len, hop, frames, scale, flags, pxy);
}

int kofft_hip_dev_csd_f32(kofft_hip_ctx *ctx, const float *d_x, const float *d_y, size_t rows, size_t len, size_t row_stride,
                          const float *d_window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_pxy)
{
    return welch_dev(ctx, true, d_x, d_y, rows, len, row_stride, d_window, win_len, hop, frames, scale, flags, d_pxy);
}

int kofft_hip_set_welch_fused(kofft_hip_ctx *ctx, int mode)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (mode < 0 || mode > 2) return KOFFT_ERR_INVALID_VALUE;
    ctx->welch_fused = mode;
    return KOFFT_OK;
}

int kofft_hip_welch_scale_f32(const float *window, size_t win_len, double fs, size_t frames, int scaling, float *scale)
{
    if (!scale) return KOFFT_ERR_NULL;
    if (win_len == 0) return KOFFT_ERR_EMPTY_INPUT;
    if ((scaling != 0 && scaling != 1) || !(fs > 0.0) || frames == 0) return KOFFT_ERR_INVALID_VALUE;
    std::vector<float> hann;
    if (!window) {
        hann.resize(win_len);
        kofft_tables::hann_f32(win_len, hann.data());
        window = hann.data();
    }
    double s = 0.0;
    for (size_t i = 0; i < win_len; ++i) {
        const double w = (double)window[i];
        s = s + (scaling == 0 ? w * w : w);
    }
    const double den = scaling == 0 ? fs * s * (double)frames : (s * s) * (double)frames;
    if (s == 0.0 || !(den == den)) return KOFFT_ERR_INVALID_VALUE;
    *scale = (float)(1.0 / den);
    return KOFFT_OK;
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

// ---- one-sided STFT over rows of signals and its inverse (k_stft_onesided.hip) ----------------------------------------
int kofft_hip_dev_stft_onesided_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                    const float *d_window, size_t win_len, size_t hop, float *d_out, size_t frames)
{
    return stft_onesided_dev(ctx, d_signal, rows, len, row_stride, d_window, win_len, hop, d_out, frames);
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
                                return stft_onesided_dev(ctx, d_in, nb, len, len, d_win, win_len, hop, d_out, frames);
                            });
}

int kofft_hip_dev_istft_onesided_f32(kofft_hip_ctx *ctx, const float *d_half, size_t rows, size_t frames, const float *d_window,
                                     size_t win_len, size_t hop, float *d_output, size_t out_len)
{
    return istft_onesided_dev(ctx, d_half, rows, frames, d_window, win_len, hop, d_output, out_len);
}

int kofft_hip_istft_onesided_f32(kofft_hip_ctx *ctx, const float *half, size_t rows, size_t frames, const float *window, size_t win_len,
                                 size_t hop, float *output, size_t out_len)
{
    const int crc = istft_rows_check(rows, frames, win_len, hop, out_len, out_len, 2);
    if (crc || rows == 0) return crc;
    // mode 2: the staged frames go up and do not come back
    return istft_stage(ctx, const_cast<float *>(half), rows, frames, window, win_len, output, out_len, nullptr, 2,
                       [&](float *d_half, const float *d_win, float *d_out, float *) {
                           return istft_onesided_dev(ctx, d_half, rows, frames, d_win, win_len, hop, d_out, out_len);
                       }, win_len / 2 + 1);
}

int kofft_hip_fftnd_c32(kofft_hip_ctx *ctx, float *data, size_t depth, size_t rows, size_t cols, int inverse)
{
    return fft_nd_host<float>(ctx, data, depth, rows, cols, inverse);
}
int kofft_hip_fftnd_c64(kofft_hip_ctx *ctx, double *data, size_t depth, size_t rows, size_t cols, int inverse)
{
    return fft_nd_host<double>(ctx, data, depth, rows, cols, inverse);
}
int kofft_hip_fftnd_c32_dev(kofft_hip_ctx *ctx, float *d_data, size_t depth, size_t rows, size_t cols, int inverse)
{
    return fft_nd_dev<float>(ctx, d_data, depth, rows, cols, inverse);
}
int kofft_hip_fftnd_c64_dev(kofft_hip_ctx *ctx, double *d_data, size_t depth, size_t rows, size_t cols, int inverse)
{
    return fft_nd_dev<double>(ctx, d_data, depth, rows, cols, inverse);
}

}  // extern "C"
