// k_mdct_f32.hip -- the fast DCT-IV of float rows, the MDCT of rows of signals and the IMDCT (mdct_impl.hip.h): every
// kernel instance of the family, its argument checks and its extern "C" entry points.
#include "mdct_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

// ---- the argument checks, in the order of include/kofft_hip.h and before the context or a device is touched ---------------------------
// N itself: shared by the three entries
static int mdct_len_check(size_t n)
{
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n & 1) return KOFFT_ERR_INVALID_VALUE;
    if (!complex_len_ok(n / 2)) return KOFFT_ERR_UNSUPPORTED;
    return KOFFT_OK;
}

// does a * b * 4 bytes stay well inside size_t (and a * b inside a signed 64-bit index)?
static bool mdct_fits(size_t a, size_t b) { return a == 0 || b <= (SIZE_MAX >> 4) / a; }

static int dct4_fast_check(size_t n, size_t batch, const void *in, const void *out, const kofft_hip_ctx *ctx)
{
    if (batch == 0) return KOFFT_OK;
    if (const int rc = mdct_len_check(n)) return rc;
    if (!mdct_fits(batch, n)) return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !in || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int mdct_check(size_t rows, size_t nx, size_t row_stride, size_t n, size_t lead, size_t frames, const void *x, const void *w, const void *out,
               const kofft_hip_ctx *ctx)
{
    if (rows == 0 || frames == 0) return KOFFT_OK;
    if (const int rc = mdct_len_check(n)) return rc;
    if (nx == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (lead >= 2 * n) return KOFFT_ERR_INVALID_VALUE;
    if (rows > 1 && row_stride < nx) return KOFFT_ERR_INVALID_VALUE;
    if (!mdct_fits(frames + 1, n) || !mdct_fits(rows, (frames + 1) * n) || !mdct_fits(rows, row_stride > nx ? row_stride : nx))
        return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !w || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int imdct_check(size_t rows, size_t frames, size_t n, size_t out_first, size_t out_len, const void *coef, const void *w, const void *out,
                const kofft_hip_ctx *ctx)
{
    if (rows == 0 || frames == 0 || out_len == 0) return KOFFT_OK;
    if (const int rc = mdct_len_check(n)) return rc;
    if (!mdct_fits(frames + 1, n) || !mdct_fits(rows, (frames + 1) * n)) return KOFFT_ERR_UNSUPPORTED;
    const size_t full = (frames + 1) * n;
    if (out_first > full || out_len > full - out_first) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (!ctx || !coef || !w || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

// ---- routes ------------------------------------------------------------------------------------------------------------------------
static bool aligned4(const void *p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }

// (the fused kernel's loads are 4 bytes wide; the route table is DESIGN.md 5.32's)
static bool dct4_fused_ok(const kofft_hip_ctx *ctx, size_t n, const void *in, const void *side)
{
    return ctx->mdct_fused && is_pow2(n) && n >= 64 && n <= 8192 && aligned4(in) && aligned4(side);
}

// dct4_fast of `items` items of policy IO, N = n, into io.out
template <class IO>
static int dct4_items(kofft_hip_ctx *ctx, const IO &io, size_t n, size_t items, bool fused)
{
    const size_t m = n / 2;
    const cpx<float> *c = nullptr;
    int rc = dct4_table(ctx, n, &c);
    if (rc) return rc;
    const cpx<float> *d = c + m;
    if (fused) {
        const cpx<float> *tw = nullptr;
        rc = twiddle_table<float>(ctx, m, &tw);  // get_twiddles(m)
        if (rc) return rc;
        return dispatch_log2<5, 12>(ilog2(m), [&](auto l) {  // (never outside 5 .. 12: dct4_fused_ok)
            constexpr int L = decltype(l)::value;
            return launch_fused_items<L>(ctx, dct4_fused_kernel<L, IO>, items, io, c, d, tw, items);
        });
    }
    // one chunk of flat items at a time (a seam may fall inside a row), scratch_chunk_bytes of scratch at most
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, m * sizeof(cpx<float>), items);
    rc = ensure(ctx, ctx->real_tmp, chunk * m * sizeof(cpx<float>));
    if (rc) return rc;
    cpx<float> *z = static_cast<cpx<float> *>(ctx->real_tmp.p);
    return for_chunks(items, chunk, [&](size_t i0, size_t ni) {
        const size_t total = ni * m;
        const dim3 grid(flat_blocks(ctx, total, 64));
        hipLaunchKernelGGL(dct4_pre_kernel<IO>, grid, dim3(256), 0, ctx->stream, io, c, z, m, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        if (m > 1) {  // (m == 1: the transform is nothing, fft.rs:1059)
            const int frc = fft_dev<float>(ctx, reinterpret_cast<float *>(z), reinterpret_cast<float *>(z), m, ni, 0);
            if (frc) return frc;
        }
        hipLaunchKernelGGL(dct4_post_kernel, grid, dim3(256), 0, ctx->stream, z, d, io.out, m, i0, total);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        return (int)KOFFT_OK;
    });
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dct4_table_f32(size_t n, float *out)
{
    if (n == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (n & 1) return KOFFT_ERR_INVALID_VALUE;
    if (!out) return KOFFT_ERR_NULL;
    kofft_tables::dct4_table_f32(n, out);
    return KOFFT_OK;
}

int kofft_hip_set_mdct_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::mdct_fused, on); }

int kofft_hip_dev_dct4_fast_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch)
{
    const int crc = dct4_fast_check(n, batch, d_in, d_out, ctx);
    if (crc || batch == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dct4_items(ctx, Dct4RowsIO{d_in, d_out, n}, n, batch, dct4_fused_ok(ctx, n, d_in, nullptr));
}

// Whole rows per chunk of the host pipeline
int kofft_hip_dct4_fast_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch)
{
    const int crc = dct4_fast_check(n, batch, in, out, ctx);
    if (crc || batch == 0) return crc;
    return rows_host<float>(ctx, in, out, batch, n, n, nullptr, 0, true, true, [&](float *d_in, float *d_out, const float *, size_t nb) {
        return kofft_hip_dev_dct4_fast_f32(ctx, d_in, d_out, n, nb);
    });
}

int kofft_hip_dev_mdct_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, size_t row_stride, const float *d_w, size_t n,
                           size_t lead, float *d_out, size_t frames)
{
    const int crc = mdct_check(rows, nx, row_stride, n, lead, frames, d_x, d_w, d_out, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const MdctIO io{d_x, d_w, d_out, n, nx, rows > 1 ? row_stride : nx, frames, lead};
    return dct4_items(ctx, io, n, rows * frames, dct4_fused_ok(ctx, n, d_x, d_w));
}

// (the window is the side input, uploaded once)
int kofft_hip_mdct_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, size_t row_stride, const float *window, size_t n, size_t lead,
                       float *out, size_t frames)
{
    const int crc = mdct_check(rows, nx, row_stride, n, lead, frames, x, window, out, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    std::vector<float> packed;
    const float *src = pack_rows(x, rows, nx, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, nx, frames * n, window, 2 * n, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return kofft_hip_dev_mdct_f32(ctx, d_in, nb, nx, nx, d_win, n, lead, d_out, frames);
                            });
}

// Chunks of the flat frame index t = row * frames + f.  The chunk [t0, t0 + nt) writes the hop blocks f of its frames (r, f), and
// block `frames` of a row with the row's last frame: every sample is written once, from frames of one chunk.  Block f > 0 needs frame
// f - 1, so a chunk that starts inside a row transforms the frame before its first as well.
int kofft_hip_dev_imdct_f32(kofft_hip_ctx *ctx, const float *d_coef, size_t rows, size_t frames, const float *d_w, size_t n, float scale,
                            float *d_out, size_t out_first, size_t out_len)
{
    const int crc = imdct_check(rows, frames, n, out_first, out_len, d_coef, d_w, d_out, ctx);
    if (crc || rows == 0 || frames == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = rows * frames, out_end = out_first + out_len;
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, n * sizeof(float), total);
    const int erc = ensure(ctx, ctx->rows_tmp, (chunk + 1) * n * sizeof(float));
    if (erc) return erc;
    float *v = static_cast<float *>(ctx->rows_tmp.p);
    const bool fused = dct4_fused_ok(ctx, n, d_coef, nullptr);
    return for_chunks(total, chunk, [&](size_t t0, size_t nt) {
        const size_t pre = t0 % frames ? 1 : 0;
        FramePiece p[3];
        const int np = frame_cut(t0, nt, frames, p);
        size_t lo[3], hi[3];
        bool any = false;
        for (int i = 0; i < np; ++i) {  // the samples of each row's `full` that the piece writes, cut to the caller's window
            const size_t last = p[i].f0 + p[i].nf, end = (last == frames ? last + 1 : last) * n;
            lo[i] = p[i].f0 * n > out_first ? p[i].f0 * n : out_first;
            hi[i] = end < out_end ? end : out_end;
            any = any || lo[i] < hi[i];
        }
        if (!any) return (int)KOFFT_OK;
        const int rc = dct4_items(ctx, Dct4RowsIO{d_coef + (t0 - pre) * n, v, n}, n, nt + pre, fused);
        if (rc) return rc;
        for (int i = 0; i < np; ++i) {
            if (lo[i] >= hi[i]) continue;
            const size_t count = p[i].nr * (hi[i] - lo[i]);
            hipLaunchKernelGGL(imdct_ola_kernel, dim3(flat_blocks(ctx, count, 64)), dim3(256), 0, ctx->stream, v + (pre + p[i].at) * n, d_w, d_out, n,
                               frames, p[i].row, p[i].f0, lo[i], hi[i], out_first, out_len, scale, count);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        return (int)KOFFT_OK;
    });
}

int kofft_hip_imdct_f32(kofft_hip_ctx *ctx, const float *coef, size_t rows, size_t frames, const float *window, size_t n, float scale, float *out,
                        size_t out_first, size_t out_len)
{
    const int crc = imdct_check(rows, frames, n, out_first, out_len, coef, window, out, ctx);
    if (crc || rows == 0 || frames == 0 || out_len == 0) return crc;
    return rows_host<float>(ctx, coef, out, rows, frames * n, out_len, window, 2 * n, true, true,
                            [&](float *d_in, float *d_out, const float *d_win, size_t nb) {
                                return kofft_hip_dev_imdct_f32(ctx, d_in, nb, frames, d_win, n, scale, d_out, out_first, out_len);
                            });
}

}  // extern "C"
