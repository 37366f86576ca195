// host_stage.hip.h -- how a host-pointer entry point reaches the device: staging (zero-copy, pipelined or serial), the row-wise forms
// of it, and the two helpers the framed families share (pack_rows, istft_stage).  Included by every k_*.hip that defines host-pointer
// entry points; everything here has internal linkage but pipeline_chunks, which kofft_hip.hip defines.
#pragma once

#include "host_common.hip.h"
#include "host_layout.h"

#include <algorithm>
#include <functional>

namespace kofft {
namespace host {

// Chunk c's upload, kernels and download of a large host batch, overlapped on three streams (kofft_hip.hip, where the helper thread
// and its headers are compiled once; a chunk costs a thread hand-off anyway, so the three indirect calls do not show):
//   up(c, stream)   -> hipError_t : enqueue chunk c's host-to-device copy on `stream`
//   run(c)          -> int        : launch chunk c's kernels on ctx->stream (status code)
//   down(c, stream) -> hipError_t : enqueue chunk c's device-to-host copy on `stream`
int pipeline_chunks(kofft_hip_ctx *ctx, size_t nchunks, const std::function<hipError_t(size_t, hipStream_t)> &up,
                    const std::function<int(size_t)> &run, const std::function<hipError_t(size_t, hipStream_t)> &down);

namespace {

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

// Host rows `row_stride` apart are packed (stride len) before they travel: the gaps are not the call's to read.
inline const float *pack_rows(const float *signal, size_t rows, size_t len, size_t row_stride, std::vector<float> &packed)
{
    if (len == 0 || rows == 1 || row_stride == len) return signal;
    packed.resize(rows * len);
    for (size_t r = 0; r < rows; ++r) std::copy_n(signal + r * row_stride, len, packed.data() + r * len);
    return packed.data();
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

}  // namespace
}  // namespace host
}  // namespace kofft
