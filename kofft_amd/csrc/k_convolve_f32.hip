// k_convolve_f32.hip -- overlap-save FFT convolution / correlation of float rows (convolve_impl.hip.h) and of rows
// against a bank of filters (convolve_bank_impl.hip.h): every kernel instance of the two families and their
// extern "C" entry points.
#include "convolve_bank_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

static size_t next_pow2(size_t v)
{
    size_t p = 1;
    while (p < v && p <= (SIZE_MAX >> 1)) p <<= 1;
    return p;
}

// The block a call with block == 0 runs with: one block per row up to 4096 points; on longer rows the smaller of
// 2048 and 4096 that leaves the filter half a block of new samples (measured: the 2048-point kernel, two frames per workgroup, beats
// the 4096-point one at 64, 512, 768 and 1024 taps), then the power of two from 2 nh.  nx, nh >= 1.
static size_t convolve_default_block(size_t nx, size_t nh)
{
    const size_t p = next_pow2(nx + nh - 1);
    if (p <= 4096) return p;
    if (nh <= 1024) return 2048;
    if (nh <= 2048) return 4096;
    const size_t q = next_pow2(2 * nh);
    return p < q ? p : q;
}

// The argument checks of both families, in the order of include/kofft_hip.h and before the context or a device is touched.  *block: 0
// on entry means the default (convolve_default_block); the block in use on return.  The families differ in three predicates, which
// the callers evaluate: `nothing` (KOFFT_OK, nothing to do), `filters_ok` and `flags_ok`.
static int conv_check(bool nothing, bool filters_ok, bool flags_ok, size_t nx, size_t nh, size_t *block, size_t out_first, size_t out_len,
                      const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    if (nothing) return KOFFT_OK;
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nx > (SIZE_MAX >> 2) || nh > (SIZE_MAX >> 2)) return KOFFT_ERR_UNSUPPORTED;  // (nx + nh - 1 and 2 nh stay inside size_t)
    if (*block == 0) *block = convolve_default_block(nx, nh);
    if (!is_pow2(*block)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (*block < nh) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (!filters_ok) return KOFFT_ERR_MISMATCHED_LENGTHS;
    const size_t full = nx + nh - 1;
    if (out_first > full || out_len > full - out_first) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (!flags_ok) return KOFFT_ERR_INVALID_VALUE;
    if (*block > kConvolveMaxBlock) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !h || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

// KOFFT_OK with rows == 0 or out_len == 0: nothing to do.
static int convolve_check(size_t rows, size_t nx, size_t nh, size_t filters, size_t *block, unsigned flags, size_t out_first, size_t out_len,
                   const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    return conv_check(rows == 0 || out_len == 0, filters == 1 || filters == rows, !(flags & ~1u), nx, nh, block, out_first, out_len, x, h, out,
                      ctx);
}

// KOFFT_OK with rows == 0, filters == 0 or out_len == 0: nothing to do.  Any number of filters; flag bits 2-3 are the output kind.
static int convolve_bank_check(size_t rows, size_t nx, size_t filters, size_t nh, size_t *block, unsigned flags, size_t out_first, size_t out_len,
                        const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    const bool flags_ok = !(flags >> (kBankKindShift + 2)) && ((flags >> kBankKindShift) & kBankKindMask) != 3u;
    return conv_check(rows == 0 || filters == 0 || out_len == 0, true, flags_ok, nx, nh, block, out_first, out_len, x, h, out, ctx);
}

// The flat items of a checked call: the nbw blocks of every row that touch the window.  false: rows * nbw does not fit size_t.
static bool convolve_shape(size_t rows, size_t nx, size_t nh, size_t block, size_t out_first, size_t out_len, bool per_row, ConvShape *s)
{
    s->nx = nx;
    s->nh = nh;
    s->hop = block - nh + 1;
    s->b0 = out_first / s->hop;
    s->nbw = (out_first + out_len - 1) / s->hop - s->b0 + 1;
    s->out_first = out_first;
    s->out_len = out_len;
    if (rows > SIZE_MAX / s->nbw) return false;
    s->items = rows * s->nbw;
    s->lb = ilog2(block);
    s->per_row = per_row;
    s->nbw32 = s->items < (size_t(1) << 31) ? (unsigned)s->nbw : 0u;
    return true;
}

// (the fused kernels' loads are 4 bytes wide; `enabled` is the context's switch of the family)
static bool conv_fused_ok(bool enabled, const float *d_x, size_t block)
{
    return enabled && block >= 32 && block <= 4096 && (reinterpret_cast<size_t>(d_x) & 3) == 0;
}

// The scratch of a call, [filters * block spectra | `bufs` buffers of chunk * block points (composed route)], and the spectra computed
// at its head: *H.  *chunk: the items per piece of the composed route, 0 on the fused one.  filters * block * 8 * (1 + bufs) fits
// size_t (the callers' checks).
static int conv_prepare(kofft_hip_ctx *ctx, const float *d_h, size_t filters, size_t nh, unsigned tap_flags, const ConvShape &s, bool fused,
                        size_t bufs, size_t *chunk, cpx<float> **H)
{
    const size_t block = size_t(1) << s.lb, total = filters * block;
    *chunk = fused ? 0 : scratch_chunk_rows(ctx->scratch_chunk_bytes, bufs * block * sizeof(cpx<float>), s.items);
    int rc = ensure(ctx, ctx->real_tmp, (total + bufs * *chunk * block) * sizeof(cpx<float>));
    if (rc) return rc;
    *H = static_cast<cpx<float> *>(ctx->real_tmp.p);
    hipLaunchKernelGGL(convolve_bank_filter_kernel, dim3(flat_blocks(ctx, total, 64)), dim3(256), 0, ctx->stream, d_h, *H, nh, s.lb, tap_flags,
                       total);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    if (block > 1) {  // (block == 1: the transform is nothing, fft.rs:1059)
        rc = fft_dev<float>(ctx, reinterpret_cast<float *>(*H), reinterpret_cast<float *>(*H), block, filters, 0);
        if (rc) return rc;
    }
    return KOFFT_OK;
}

// The composed routes' first half for items [i0, i0 + ni): their frames as (x, +0) into X, transformed in place.
static int conv_frames(kofft_hip_ctx *ctx, const float *d_x, cpx<float> *X, const ConvShape &s, size_t i0, size_t ni, dim3 grid)
{
    const size_t block = size_t(1) << s.lb;
    hipLaunchKernelGGL(convolve_expand_kernel, grid, dim3(256), 0, ctx->stream, d_x, X, s, i0, ni * block);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    if (block == 1) return KOFFT_OK;  // (the transform is nothing, fft.rs:1059)
    return fft_dev<float>(ctx, reinterpret_cast<float *>(X), reinterpret_cast<float *>(X), block, ni, 0);
}

// ... and their last steps for the products y of one filter: ifft in place, then the kept parts into the window of (row, filter f)
template <class Kind>
static int conv_finish(kofft_hip_ctx *ctx, cpx<float> *y, void *d_out, const ConvShape &s, size_t filters, size_t f, size_t i0, size_t ni,
                       dim3 grid)
{
    const size_t block = size_t(1) << s.lb;
    if (block > 1) {  // (block == 1: ifft returns early, fft.rs:1139)
        const int rc = fft_dev<float>(ctx, reinterpret_cast<float *>(y), reinterpret_cast<float *>(y), block, ni, 1);  // conj, fft, conj * (1 / block)
        if (rc) return rc;
    }
    hipLaunchKernelGGL(convolve_bank_gather_kernel<Kind>, grid, dim3(256), 0, ctx->stream, y, static_cast<typename Kind::Out *>(d_out), s, filters,
                       f, i0, ni * block);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// One chunk of flat items at a time (a seam may fall inside a row), all in one buffer z.
static int convolve_composed(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, cpx<float> *z, size_t chunk, float *d_out,
                             const ConvShape &s)
{
    return for_chunks(s.items, chunk, [&](size_t i0, size_t ni) {
        const size_t total = ni << s.lb;
        const dim3 grid(flat_blocks(ctx, total, 64));
        const int rc = conv_frames(ctx, d_x, z, s, i0, ni, grid);
        if (rc) return rc;
        hipLaunchKernelGGL(convolve_mul_kernel, grid, dim3(256), 0, ctx->stream, z, H, s, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return conv_finish<BankReal>(ctx, z, d_out, s, 1, 0, i0, ni, grid);
    });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_set_convolve_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::convolve_fused, on); }
int kofft_hip_set_convolve_bank_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::convolve_bank_fused, on); }

int kofft_hip_convolve_block(size_t nx, size_t nh, size_t *block)
{
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nx > (SIZE_MAX >> 2) || nh > (SIZE_MAX >> 2)) return KOFFT_ERR_UNSUPPORTED;
    if (!block) return KOFFT_ERR_NULL;
    *block = convolve_default_block(nx, nh);
    return KOFFT_OK;
}

int kofft_hip_dev_convolve_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                               size_t block, unsigned flags, float *d_out, size_t out_first, size_t out_len)
{
    const int crc = convolve_check(rows, nx, nh, filters, &block, flags, out_first, out_len, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ConvShape s{};
    if (!convolve_shape(rows, nx, nh, block, out_first, out_len, filters == rows && rows > 1, &s)) return KOFFT_ERR_UNSUPPORTED;
    if (filters > (SIZE_MAX >> 4) / block) return KOFFT_ERR_UNSUPPORTED;
    const bool fused = conv_fused_ok(ctx->convolve_fused, d_x, block);
    size_t chunk = 0;
    cpx<float> *H = nullptr;
    int rc = conv_prepare(ctx, d_h, filters, nh, flags & kBankCorrelate, s, fused, 1, &chunk, &H);
    if (rc) return rc;
    if (!fused) return convolve_composed(ctx, d_x, H, H + filters * block, chunk, d_out, s);
    const cpx<float> *tw = nullptr;
    rc = twiddle_table<float>(ctx, block, &tw);  // get_twiddles(block)
    if (rc) return rc;
    return dispatch_log2<5, 12>(s.lb, [&](auto l) {  // (never outside 5 .. 12: conv_fused_ok)
        constexpr int L = decltype(l)::value;
        return launch_fused_items<L>(ctx, convolve_fused_kernel<L>, s.items, d_x, H, d_out, tw, s);
    });
}

// On host rows: nx samples in, out_len values out.  One filter for all rows is the side input, uploaded once; one filter per row is a
// third array, so that a pipelined chunk carries its own rows' taps
int kofft_hip_convolve_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh, size_t block,
                           unsigned flags, float *out, size_t out_first, size_t out_len)
{
    const int crc = convolve_check(rows, nx, nh, filters, &block, flags, out_first, out_len, x, h, out, ctx);
    if (crc || rows == 0 || out_len == 0) return crc;
    if (filters == rows && rows > 1) {
        const HostArray<float> a[3] = {{x, nullptr, nx}, {h, nullptr, nh}, {nullptr, out, out_len}};
        return rows_host_n<float>(ctx, rows, 3, a, nullptr, 0, true, true, [&](float *const *d, const float *, size_t nr) {
            return kofft_hip_dev_convolve_f32(ctx, d[0], nr, nx, d[1], nr, nh, block, flags, d[2], out_first, out_len);
        });
    }
    return rows_host<float>(ctx, x, out, rows, nx, out_len, h, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return kofft_hip_dev_convolve_f32(ctx, d_in, nr, nx, d_h, 1, nh, block, flags, d_out, out_first, out_len);
                            });
}

}  // extern "C"

// ---- the filter bank ---------------------------------------------------------------------------------------------
// One chunk of flat items at a time: the frames and their transforms once into X, then every filter through y.
template <class Kind>
static int convolve_bank_composed(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, cpx<float> *X, size_t chunk, void *d_out,
                                  const ConvShape &s, size_t filters)
{
    cpx<float> *y = X + (chunk << s.lb);
    return for_chunks(s.items, chunk, [&](size_t i0, size_t ni) {
        const size_t total = ni << s.lb;
        const dim3 grid(flat_blocks(ctx, total, 64));
        const int rc = conv_frames(ctx, d_x, X, s, i0, ni, grid);
        if (rc) return rc;
        for (size_t f = 0; f < filters; ++f) {
            hipLaunchKernelGGL(convolve_bank_mul_kernel, grid, dim3(256), 0, ctx->stream, X, H + (f << s.lb), y, s.lb, total);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
            const int frc = conv_finish<Kind>(ctx, y, d_out, s, filters, f, i0, ni, grid);
            if (frc) return frc;
        }
        return KOFFT_OK;
    });
}

template <class Kind>
static int convolve_bank_route(kofft_hip_ctx *ctx, const float *d_x, cpx<float> *H, void *d_out, const ConvShape &s, size_t filters,
                               bool fused, size_t chunk)
{
    const size_t block = size_t(1) << s.lb;
    if (!fused) return convolve_bank_composed<Kind>(ctx, d_x, H, H + filters * block, chunk, d_out, s, filters);
    const cpx<float> *tw = nullptr;
    const int rc = twiddle_table<float>(ctx, block, &tw);  // get_twiddles(block)
    if (rc) return rc;
    return dispatch_log2<5, 12>(s.lb, [&](auto l) {  // (never outside 5 .. 12: conv_fused_ok)
        constexpr int L = decltype(l)::value;
        return launch_fused_items<L>(ctx, convolve_bank_fused_kernel<L, Kind>, s.items, d_x, H, static_cast<typename Kind::Out *>(d_out), tw, s,
                                     filters);
    });
}

extern "C" {

int kofft_hip_dev_convolve_bank_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                                    size_t block, unsigned flags, void *d_out, size_t out_first, size_t out_len)
{
    const int crc = convolve_bank_check(rows, nx, filters, nh, &block, flags, out_first, out_len, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || filters == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ConvShape s{};
    if (!convolve_shape(rows, nx, nh, block, out_first, out_len, false, &s)) return KOFFT_ERR_UNSUPPORTED;
    if (filters > (SIZE_MAX >> 5) / block || rows > (SIZE_MAX >> 3) / filters / out_len) return KOFFT_ERR_UNSUPPORTED;
    const bool fused = conv_fused_ok(ctx->convolve_bank_fused, d_x, block);
    size_t chunk = 0;
    cpx<float> *H = nullptr;
    // (two buffers per chunk on the composed route: the transformed frames, which stay for the next filter, and the products)
    const int rc = conv_prepare(ctx, d_h, filters, nh, flags & (kBankCorrelate | kBankComplexTaps), s, fused, 2, &chunk, &H);
    if (rc) return rc;
    switch ((flags >> kBankKindShift) & kBankKindMask) {
    case 0: return convolve_bank_route<BankReal>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    case 1: return convolve_bank_route<BankComplex>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    default: return convolve_bank_route<BankMagnitude>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    }
}


// On host rows: the bank is the side input, uploaded once; a row of the output is filters * out_len elements of one or (complex
// values) two floats
int kofft_hip_convolve_bank_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh,
                                size_t block, unsigned flags, void *out, size_t out_first, size_t out_len)
{
    const int crc = convolve_bank_check(rows, nx, filters, nh, &block, flags, out_first, out_len, x, h, out, ctx);
    if (crc || rows == 0 || filters == 0 || out_len == 0) return crc;
    if (filters > (SIZE_MAX >> 3) / nh || filters > (SIZE_MAX >> 3) / out_len) return KOFFT_ERR_UNSUPPORTED;
    const size_t out_row = filters * out_len * (((flags >> 2) & 3u) == 1u ? 2 : 1), side_len = filters * nh * ((flags & 2u) ? 2 : 1);
    return rows_host<float>(ctx, x, static_cast<float *>(out), rows, nx, out_row, h, side_len, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nr) {
                                return kofft_hip_dev_convolve_bank_f32(ctx, d_in, nr, nx, d_h, filters, nh, block, flags, d_out, out_first, out_len);
                            });
}

}  // extern "C"
