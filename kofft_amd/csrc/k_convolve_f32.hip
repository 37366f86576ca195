// k_convolve_f32.hip -- overlap-save FFT convolution / correlation of float rows (convolve_impl.hip.h) and of rows
// against a bank of filters (convolve_bank_impl.hip.h): every kernel instance of the two families and their
// device-pointer entry points.
#include "convolve_bank_impl.hip.h"

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
size_t convolve_default_block(size_t nx, size_t nh)
{
    const size_t p = next_pow2(nx + nh - 1);
    if (p <= 4096) return p;
    if (nh <= 1024) return 2048;
    if (nh <= 2048) return 4096;
    const size_t q = next_pow2(2 * nh);
    return p < q ? p : q;
}

// The argument checks alone, in the order of include/kofft_hip.h and before the context or a device is touched.  *block: 0 on entry
// means the default (convolve_default_block); the block in use on return.  KOFFT_OK with rows == 0 or out_len == 0: nothing to do.
int convolve_check(size_t rows, size_t nx, size_t nh, size_t filters, size_t *block, unsigned flags, size_t out_first, size_t out_len,
                   const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    if (rows == 0 || out_len == 0) return KOFFT_OK;
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nx > (SIZE_MAX >> 2) || nh > (SIZE_MAX >> 2)) return KOFFT_ERR_UNSUPPORTED;  // (nx + nh - 1 and 2 nh stay inside size_t)
    if (*block == 0) *block = convolve_default_block(nx, nh);
    if (!is_pow2(*block)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (*block < nh) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (filters != 1 && filters != rows) return KOFFT_ERR_MISMATCHED_LENGTHS;
    const size_t full = nx + nh - 1;
    if (out_first > full || out_len > full - out_first) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (flags & ~1u) return KOFFT_ERR_INVALID_VALUE;
    if (*block > kConvolveMaxBlock) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !h || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int convolve_composed(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, cpx<float> *z, size_t chunk, float *d_out,
                             const ConvShape &s)
{
    const size_t block = size_t(1) << s.lb;
    float *zf = reinterpret_cast<float *>(z);
    for (size_t i0 = 0; i0 < s.items; i0 += chunk) {
        const size_t ni = (s.items - i0 < chunk) ? s.items - i0 : chunk, total = ni * block;
        const dim3 grid(hilbert_flat_blocks(ctx, total));
        hipLaunchKernelGGL(convolve_expand_kernel, grid, dim3(256), 0, ctx->stream, d_x, z, s, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (block > 1) {  // (block == 1: the transform is nothing, fft.rs:1059)
            const int rc = fft_dev<float>(ctx, zf, zf, block, ni, 0);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(convolve_mul_kernel, grid, dim3(256), 0, ctx->stream, z, H, s, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (block > 1) {  // (block == 1: ifft returns early, fft.rs:1139)
            const int rc = fft_dev<float>(ctx, zf, zf, block, ni, 1);  // conj, fft, conj * (1 / block)
            if (rc) return rc;
        }
        hipLaunchKernelGGL(convolve_gather_kernel, grid, dim3(256), 0, ctx->stream, z, d_out, s, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
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

int convolve_dev(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh, size_t block,
                 unsigned flags, float *d_out, size_t out_first, size_t out_len)
{
    const int crc = convolve_check(rows, nx, nh, filters, &block, flags, out_first, out_len, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ConvShape s{};
    if (!convolve_shape(rows, nx, nh, block, out_first, out_len, filters == rows && rows > 1, &s)) return KOFFT_ERR_UNSUPPORTED;
    const bool fused = ctx->convolve_fused && block >= 32 && block <= 4096 && (reinterpret_cast<size_t>(d_x) & 3) == 0;
    // scratch: [filters * block spectra | chunk * block frames (composed route)]
    if (filters > (SIZE_MAX >> 4) / block) return KOFFT_ERR_UNSUPPORTED;
    const size_t h_bytes = filters * block * sizeof(cpx<float>);
    const size_t chunk = fused ? 0 : scratch_chunk_rows(ctx->scratch_chunk_bytes, block * sizeof(cpx<float>), s.items);
    int rc = ensure(ctx, ctx->real_tmp, h_bytes + chunk * block * sizeof(cpx<float>));
    if (rc) return rc;
    cpx<float> *H = static_cast<cpx<float> *>(ctx->real_tmp.p);
    {
        const size_t total = filters * block;
        hipLaunchKernelGGL(convolve_filter_kernel, dim3(hilbert_flat_blocks(ctx, total)), dim3(256), 0, ctx->stream, d_h, H, nh, s.lb,
                           (int)(flags & 1u), total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (block > 1) {
            rc = fft_dev<float>(ctx, reinterpret_cast<float *>(H), reinterpret_cast<float *>(H), block, filters, 0);
            if (rc) return rc;
        }
    }
    if (!fused) return convolve_composed(ctx, d_x, H, H + filters * block, chunk, d_out, s);
    const cpx<float> *tw = nullptr;
    rc = twiddle_table<float>(ctx, block, &tw);  // get_twiddles(block)
    if (rc) return rc;
    switch (s.lb) {
    case 5: return launch_convolve_fused<5>(ctx, d_x, H, d_out, tw, s);
    case 6: return launch_convolve_fused<6>(ctx, d_x, H, d_out, tw, s);
    case 7: return launch_convolve_fused<7>(ctx, d_x, H, d_out, tw, s);
    case 8: return launch_convolve_fused<8>(ctx, d_x, H, d_out, tw, s);
    case 9: return launch_convolve_fused<9>(ctx, d_x, H, d_out, tw, s);
    case 10: return launch_convolve_fused<10>(ctx, d_x, H, d_out, tw, s);
    case 11: return launch_convolve_fused<11>(ctx, d_x, H, d_out, tw, s);
    case 12: return launch_convolve_fused<12>(ctx, d_x, H, d_out, tw, s);
    default: return KOFFT_ERR_UNSUPPORTED;  // (never: `fused`)
    }
}

// ---- the filter bank ---------------------------------------------------------------------------------------------
// The argument checks alone, in the order of include/kofft_hip.h and before the context or a device is touched; *block as in
// convolve_check.
int convolve_bank_check(size_t rows, size_t nx, size_t filters, size_t nh, size_t *block, unsigned flags, size_t out_first, size_t out_len,
                        const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    if (rows == 0 || filters == 0 || out_len == 0) return KOFFT_OK;
    if (nx == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nx > (SIZE_MAX >> 2) || nh > (SIZE_MAX >> 2)) return KOFFT_ERR_UNSUPPORTED;  // (nx + nh - 1 and 2 nh stay inside size_t)
    if (*block == 0) *block = convolve_default_block(nx, nh);
    if (!is_pow2(*block)) return KOFFT_ERR_NON_POWER_OF_TWO_NO_STD;
    if (*block < nh) return KOFFT_ERR_MISMATCHED_LENGTHS;
    const size_t full = nx + nh - 1;
    if (out_first > full || out_len > full - out_first) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if ((flags >> (kBankKindShift + 2)) || ((flags >> kBankKindShift) & kBankKindMask) == 3u) return KOFFT_ERR_INVALID_VALUE;
    if (*block > kConvolveMaxBlock) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !h || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

// One chunk of flat items at a time: the frames and their transforms once into X, then every filter through y.
template <class Kind>
static int convolve_bank_composed(kofft_hip_ctx *ctx, const float *d_x, const cpx<float> *H, cpx<float> *X, size_t chunk, void *d_out,
                                  const ConvShape &s, size_t filters)
{
    const size_t block = size_t(1) << s.lb;
    cpx<float> *y = X + chunk * block;
    float *Xf = reinterpret_cast<float *>(X), *yf = reinterpret_cast<float *>(y);
    for (size_t i0 = 0; i0 < s.items; i0 += chunk) {
        const size_t ni = (s.items - i0 < chunk) ? s.items - i0 : chunk, total = ni * block;
        const dim3 grid(hilbert_flat_blocks(ctx, total));
        hipLaunchKernelGGL(convolve_expand_kernel, grid, dim3(256), 0, ctx->stream, d_x, X, s, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (block > 1) {  // (block == 1: the transform is nothing, fft.rs:1059)
            const int rc = fft_dev<float>(ctx, Xf, Xf, block, ni, 0);
            if (rc) return rc;
        }
        for (size_t f = 0; f < filters; ++f) {
            hipLaunchKernelGGL(convolve_bank_mul_kernel, grid, dim3(256), 0, ctx->stream, X, H + f * block, y, s.lb, total);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
            if (block > 1) {  // (block == 1: ifft returns early, fft.rs:1139)
                const int rc = fft_dev<float>(ctx, yf, yf, block, ni, 1);  // conj, fft, conj * (1 / block)
                if (rc) return rc;
            }
            hipLaunchKernelGGL(convolve_bank_gather_kernel<Kind>, grid, dim3(256), 0, ctx->stream, y, static_cast<typename Kind::Out *>(d_out),
                               s, filters, f, i0, total);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
    }
    return KOFFT_OK;
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
    switch (s.lb) {
    case 5: return launch_convolve_bank_fused<5, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 6: return launch_convolve_bank_fused<6, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 7: return launch_convolve_bank_fused<7, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 8: return launch_convolve_bank_fused<8, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 9: return launch_convolve_bank_fused<9, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 10: return launch_convolve_bank_fused<10, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 11: return launch_convolve_bank_fused<11, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    case 12: return launch_convolve_bank_fused<12, Kind>(ctx, d_x, H, d_out, tw, s, filters);
    default: return KOFFT_ERR_UNSUPPORTED;  // (never: `fused`)
    }
}

int convolve_bank_dev(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh, size_t block,
                      unsigned flags, void *d_out, size_t out_first, size_t out_len)
{
    const int crc = convolve_bank_check(rows, nx, filters, nh, &block, flags, out_first, out_len, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || filters == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ConvShape s{};
    if (!convolve_shape(rows, nx, nh, block, out_first, out_len, false, &s)) return KOFFT_ERR_UNSUPPORTED;
    if (filters > (SIZE_MAX >> 5) / block || rows > (SIZE_MAX >> 3) / filters / out_len) return KOFFT_ERR_UNSUPPORTED;
    const bool fused = ctx->convolve_bank_fused && block >= 32 && block <= 4096 && (reinterpret_cast<size_t>(d_x) & 3) == 0;
    // scratch: [filters * block spectra | chunk * block transformed frames | chunk * block products (composed route)]
    const size_t h_bytes = filters * block * sizeof(cpx<float>);
    const size_t chunk = fused ? 0 : scratch_chunk_rows(ctx->scratch_chunk_bytes, 2 * block * sizeof(cpx<float>), s.items);
    int rc = ensure(ctx, ctx->real_tmp, h_bytes + 2 * chunk * block * sizeof(cpx<float>));
    if (rc) return rc;
    cpx<float> *H = static_cast<cpx<float> *>(ctx->real_tmp.p);
    {
        const size_t total = filters * block;
        hipLaunchKernelGGL(convolve_bank_filter_kernel, dim3(hilbert_flat_blocks(ctx, total)), dim3(256), 0, ctx->stream, d_h, H, nh, s.lb,
                           flags & (kBankCorrelate | kBankComplexTaps), total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (block > 1) {
            rc = fft_dev<float>(ctx, reinterpret_cast<float *>(H), reinterpret_cast<float *>(H), block, filters, 0);
            if (rc) return rc;
        }
    }
    switch ((flags >> kBankKindShift) & kBankKindMask) {
    case 0: return convolve_bank_route<BankReal>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    case 1: return convolve_bank_route<BankComplex>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    default: return convolve_bank_route<BankMagnitude>(ctx, d_x, H, d_out, s, filters, fused, chunk);
    }
}

}  // namespace host
}  // namespace kofft
