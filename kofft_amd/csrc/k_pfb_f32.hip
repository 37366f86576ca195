// k_pfb_f32.hip -- the polyphase filter bank of float rows, analysis and synthesis (pfb_impl.hip.h): every kernel
// instance of the family, its argument checks, its two host helpers and its extern "C" entry points.
#include "pfb_impl.hip.h"
#include "host_stage.hip.h"
#include "kaiser_i0.h"

#include <cmath>

namespace kofft {
namespace host {

// ---- the argument checks, in the order of include/kofft_hip.h and before the context or a device is touched ---------------------------
// does a * b * 16 bytes stay inside size_t (and a * b inside a signed 64-bit index)?
static bool pfb_fits(size_t a, size_t b) { return a == 0 || b <= (SIZE_MAX >> 4) / a; }

// M, nh, bins and D: shared by the two directions (synthesis: bins is M or the one-sided M/2 + 1)
static int pfb_shape_check(size_t nh, size_t m, size_t d, size_t bins, bool synthesis)
{
    if (m == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nh % m != 0 || bins == 0 || bins > m) return KOFFT_ERR_INVALID_VALUE;
    if (synthesis && bins != m && !(m % 2 == 0 && bins == m / 2 + 1)) return KOFFT_ERR_INVALID_VALUE;
    if (!complex_len_ok(m)) return KOFFT_ERR_UNSUPPORTED;
    if (d == 0) return KOFFT_ERR_INVALID_HOP_SIZE;
    return KOFFT_OK;
}

static int pfb_analysis_check(size_t rows, size_t nx, size_t row_stride, size_t nh, size_t m, size_t d, size_t lead, size_t frames, size_t bins,
                              const void *x, const void *h, const void *out, const kofft_hip_ctx *ctx)
{
    if (rows == 0 || frames == 0) return KOFFT_OK;
    if (const int rc = pfb_shape_check(nh, m, d, bins, false)) return rc;
    if (nx == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (lead >= nh) return KOFFT_ERR_INVALID_VALUE;
    if (rows > 1 && row_stride < nx) return KOFFT_ERR_INVALID_VALUE;
    // frames * D + nh (the last sample index a frame names), rows * frames * M (the composed route's scratch) and the rows themselves
    if (!pfb_fits(frames, d) || nh > (SIZE_MAX >> 4) - frames * d || !pfb_fits(frames, m) || !pfb_fits(rows, frames * m) ||
        !pfb_fits(rows, row_stride > nx ? row_stride : nx))
        return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !h || !out) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

static int pfb_synthesis_check(size_t rows, size_t frames, size_t bins, size_t nh, size_t m, size_t d, size_t out_first, size_t out_len,
                               const void *spec, const void *g, const void *out, const kofft_hip_ctx *ctx)
{
    if (rows == 0 || frames == 0) return KOFFT_OK;
    if (const int rc = pfb_shape_check(nh, m, d, bins, true)) return rc;
    if (!pfb_fits(frames, d) || nh > (SIZE_MAX >> 4) - frames * d || !pfb_fits(frames, m) || !pfb_fits(rows, frames * m) ||
        !pfb_fits(rows, (frames - 1) * d + nh))
        return KOFFT_ERR_UNSUPPORTED;
    const size_t full = (frames - 1) * d + nh;
    if (out_first > full || out_len > full - out_first) return KOFFT_ERR_MISMATCHED_LENGTHS;
    if (!ctx || !spec || !g || (out_len && !out)) return KOFFT_ERR_NULL;
    return KOFFT_OK;
}

// ---- routes ------------------------------------------------------------------------------------------------------------------------
static bool aligned4(const void *p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }

// The measured choice of the default context: the fused analysis kernel wins up to M = 1024 and loses to the composed
// route at 2048 and 4096, where one workgroup per frame leaves too few loads in flight; the fused inverse wins at every M it covers.
static bool pfb_use_fused(size_t m, bool analysis) { return !analysis || m <= 1024; }

// (the fused kernels exist for M = 32 .. 4096 and their real loads are 4 bytes wide)
static bool pfb_fused_ok(const kofft_hip_ctx *ctx, size_t m, const void *in, const void *side, bool analysis)
{
    if (ctx->pfb_fused == 0 || !is_pow2(m) || m < 32 || m > 4096 || !aligned4(in) || !aligned4(side)) return false;
    return ctx->pfb_fused == 2 || pfb_use_fused(m, analysis);
}

// the analysis of `items` flat items of io into io.out
static int pfb_analysis_items(kofft_hip_ctx *ctx, const PfbIO &io, size_t items, bool fused)
{
    const size_t m = io.m, bins = io.bins;
    if (fused) {
        const cpx<float> *tw = nullptr;
        const int rc = twiddle_table<float>(ctx, m, &tw);  // get_twiddles(M)
        if (rc) return rc;
        return dispatch_log2<5, 12>(ilog2(m), [&](auto l) {  // (never outside 5 .. 12: pfb_fused_ok)
            constexpr int L = decltype(l)::value;
            return launch_fused_items<L>(ctx, pfb_fused_kernel<L, PfbIO>, items, io, tw, items);
        });
    }
    // one chunk of flat items at a time (a seam may fall inside a row), scratch_chunk_bytes of scratch at most
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, m * sizeof(cpx<float>), items);
    const int erc = ensure(ctx, ctx->real_tmp, chunk * m * sizeof(cpx<float>));
    if (erc) return erc;
    cpx<float> *z = static_cast<cpx<float> *>(ctx->real_tmp.p);
    return for_chunks(items, chunk, [&](size_t i0, size_t ni) {
        hipLaunchKernelGGL(pfb_fold_kernel<PfbIO>, dim3(flat_blocks(ctx, ni * m, 64)), dim3(256), 0, ctx->stream, io, z, i0, ni * m);
        KOFFT_HIP_TRY(ctx, hipGetLastError());
        cpx<float> *dst = io.out + i0 * bins;
        const bool direct = bins == m;  // the transform goes straight to the caller's frames
        if (m > 1) {                    // (M == 1: the transform is nothing, fft.rs:1059)
            const int frc = fft_dev<float>(ctx, reinterpret_cast<const float *>(z), reinterpret_cast<float *>(direct ? dst : z), m, ni, 0);
            if (frc) return frc;
        }
        if (!direct || m == 1) {
            hipLaunchKernelGGL(pfb_prefix_kernel, dim3(flat_blocks(ctx, ni * bins, 64)), dim3(256), 0, ctx->stream, z, dst, m, bins, ni * bins);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        return (int)KOFFT_OK;
    });
}

// v[q][j] = ifft(F_q)[j].re for the `items` frames at spec, M reals per frame
static int pfb_inverse_items(kofft_hip_ctx *ctx, const cpx<float> *spec, float *v, cpx<float> *z, size_t m, size_t bins, size_t items, bool fused)
{
    if (fused) {
        const cpx<float> *tw = nullptr;
        const int rc = twiddle_table<float>(ctx, m, &tw);
        if (rc) return rc;
        return dispatch_log2<5, 12>(ilog2(m), [&](auto l) {
            constexpr int L = decltype(l)::value;
            return launch_fused_items<L>(ctx, pfb_inverse_fused_kernel<L>, items, spec, v, bins, tw, items);
        });
    }
    const dim3 grid(flat_blocks(ctx, items * m, 64));
    hipLaunchKernelGGL(pfb_complete_kernel, grid, dim3(256), 0, ctx->stream, spec, z, m, bins, items * m);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    if (m > 1) {  // (M == 1: ifft returns early)
        const int frc = fft_dev<float>(ctx, reinterpret_cast<const float *>(z), reinterpret_cast<float *>(z), m, items, 1);
        if (frc) return frc;
    }
    hipLaunchKernelGGL(pfb_real_kernel, grid, dim3(256), 0, ctx->stream, z, v, items * m);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

// sinc((i - (nh - 1) / 2) / M) under a Kaiser window of `beta`, normalised to unit sum: double throughout, rounded to f32 once
int kofft_hip_pfb_taps_f32(size_t m, size_t taps, double beta, float *out)
{
    if (m == 0 || taps == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (!(beta >= 0.0)) return KOFFT_ERR_INVALID_VALUE;
    if (!out) return KOFFT_ERR_NULL;
    size_t nh = 0;
    if (__builtin_mul_overflow(m, taps, &nh) || nh > (size_t(1) << 28)) return KOFFT_ERR_UNSUPPORTED;
    std::vector<double> h;
    try {
        h.resize(nh);
    } catch (const std::bad_alloc &) {
        return KOFFT_ERR_ALLOC;
    }
    const double mid = ((double)nh - 1.0) / 2.0, i0b = bessel_i0(beta);
    double sum = 0.0;
    for (size_t i = 0; i < nh; ++i) {
        const double c = (double)i - mid;
        const double y = M_PI * (c / (double)m);
        const double sinc = y == 0.0 ? 1.0 : std::sin(y) / y;
        const double r = mid > 0.0 ? c / mid : 0.0, inside = 1.0 - r * r;
        const double w = bessel_i0(beta * std::sqrt(inside > 0.0 ? inside : 0.0)) / i0b;
        h[i] = sinc * w;
        sum = sum + h[i];
    }
    for (size_t i = 0; i < nh; ++i) out[i] = (float)(h[i] / sum);
    return KOFFT_OK;
}

// For every p mod D and every q: sum over the frames f that cover p of g[n_f] * h[n_f + qM], n_f = p - fD -- c * delta[q] where
// synthesis(analysis(x)) is c * x.  Since n_f runs over the taps n == p (mod D), p in [0, D) covers every class.
int kofft_hip_pfb_reconstruction(const float *h, const float *g, size_t nh, size_t m, size_t d, double *c, double *worst)
{
    if (m == 0 || nh == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (nh % m != 0) return KOFFT_ERR_INVALID_VALUE;
    if (d == 0) return KOFFT_ERR_INVALID_HOP_SIZE;
    if (!h || !g || !c || !worst) return KOFFT_ERR_NULL;
    const long long taps = (long long)(nh / m);
    auto sum = [&](size_t p, long long q) {
        double s = 0.0;
        for (size_t n = p; n < nh; n += d) {
            const long long i = (long long)n + q * (long long)m;
            if (i >= 0 && i < (long long)nh) s = s + (double)g[n] * (double)h[i];
        }
        return s;
    };
    const double c0 = sum(0, 0);
    double w = 0.0;
    const size_t classes = d < nh ? d : nh;
    for (size_t p = 0; p < classes; ++p)
        for (long long q = -(taps - 1); q <= taps - 1; ++q) {
            const double dev = std::fabs(sum(p, q) - (q == 0 ? c0 : 0.0));
            if (!(dev <= w)) w = dev;  // (a NaN stays)
        }
    *c = c0;
    *worst = w;
    return KOFFT_OK;
}

int kofft_hip_set_pfb_fused(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::pfb_fused, on, 0, 2); }

int kofft_hip_dev_pfb_analysis_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, size_t row_stride, const float *d_h, size_t nh,
                                   size_t m, size_t d, size_t lead, float *d_out, size_t frames, size_t bins)
{
    const int crc = pfb_analysis_check(rows, nx, row_stride, nh, m, d, lead, frames, bins, d_x, d_h, d_out, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PfbIO io{d_x, d_h, reinterpret_cast<cpx<float> *>(d_out), m, nh / m, nx, rows > 1 ? row_stride : nx, frames, d, lead, bins};
    return pfb_analysis_items(ctx, io, rows * frames, pfb_fused_ok(ctx, m, d_x, d_h, true));
}

// (the taps are the side input, uploaded once; whole rows per chunk of the host pipeline)
int kofft_hip_pfb_analysis_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, size_t row_stride, const float *h, size_t nh, size_t m,
                               size_t d, size_t lead, float *out, size_t frames, size_t bins)
{
    const int crc = pfb_analysis_check(rows, nx, row_stride, nh, m, d, lead, frames, bins, x, h, out, ctx);
    if (crc || rows == 0 || frames == 0) return crc;
    std::vector<float> packed;
    const float *src = pack_rows(x, rows, nx, row_stride, packed);
    return rows_host<float>(ctx, src, out, rows, nx, frames * bins * 2, h, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_h, size_t nb) {
                                return kofft_hip_dev_pfb_analysis_f32(ctx, d_in, nb, nx, nx, d_h, nh, m, d, lead, d_out, frames, bins);
                            });
}

// Chunks of the flat frame index t = row * frames + f.  Frame f of a row owns the samples [fD, (f + 1)D) of the row's `full`, the last
// frame the rest: every sample is written once, by the chunk that holds its last covering frame (a sample that no frame covers, D >
// nh, by the frame before the gap).  A sample of frame f's needs the frames down to f - (ceil(nh / D) - 1), so a chunk that starts
// inside a row transforms up to that many frames before its first as well.
int kofft_hip_dev_pfb_synthesis_f32(kofft_hip_ctx *ctx, const float *d_spec, size_t rows, size_t frames, size_t bins, const float *d_g, size_t nh,
                                    size_t m, size_t d, float scale, float *d_out, size_t out_first, size_t out_len)
{
    const int crc = pfb_synthesis_check(rows, frames, bins, nh, m, d, out_first, out_len, d_spec, d_g, d_out, ctx);
    if (crc || rows == 0 || frames == 0 || out_len == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = rows * frames, out_end = out_first + out_len, full = (frames - 1) * d + nh;
    size_t back = (nh + d - 1) / d - 1;  // frames before a chunk's first that its samples may need
    if (back > frames - 1) back = frames - 1;
    const bool fused = pfb_fused_ok(ctx, m, d_spec, nullptr, false);
    const size_t chunk = scratch_chunk_rows(ctx->scratch_chunk_bytes, m * (fused ? sizeof(float) : sizeof(cpx<float>)), total);
    if (!pfb_fits(chunk + back, m)) return KOFFT_ERR_UNSUPPORTED;
    int erc = ensure(ctx, ctx->rows_tmp, (chunk + back) * m * sizeof(float));
    if (!erc && !fused) erc = ensure(ctx, ctx->real_tmp, (chunk + back) * m * sizeof(cpx<float>));
    if (erc) return erc;
    float *v = static_cast<float *>(ctx->rows_tmp.p);
    cpx<float> *z = static_cast<cpx<float> *>(ctx->real_tmp.p);
    const cpx<float> *spec = reinterpret_cast<const cpx<float> *>(d_spec);
    return for_chunks(total, chunk, [&](size_t t0, size_t nt) {
        const size_t f_first = t0 % frames, pre = f_first < back ? f_first : back;
        FramePiece p[3];
        const int np = frame_cut(t0, nt, frames, p);
        size_t lo[3], hi[3];
        bool any = false;
        for (int i = 0; i < np; ++i) {  // the samples of each row's `full` that the piece writes, cut to the caller's window
            const size_t last = p[i].f0 + p[i].nf, end = last == frames ? full : last * d;
            lo[i] = p[i].f0 * d > out_first ? p[i].f0 * d : out_first;
            hi[i] = end < out_end ? end : out_end;
            any = any || lo[i] < hi[i];
        }
        if (!any) return (int)KOFFT_OK;
        const int rc = pfb_inverse_items(ctx, spec + (t0 - pre) * bins, v, z, m, bins, nt + pre, fused);
        if (rc) return rc;
        for (int i = 0; i < np; ++i) {
            if (lo[i] >= hi[i]) continue;
            const size_t count = p[i].nr * (hi[i] - lo[i]);
            hipLaunchKernelGGL(pfb_ola_kernel, dim3(flat_blocks(ctx, count, 64)), dim3(256), 0, ctx->stream, v + (pre + p[i].at) * m, d_g, d_out, m, nh,
                               d, frames, p[i].row, p[i].f0, lo[i], hi[i], out_first, out_len, scale, count);
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        return (int)KOFFT_OK;
    });
}

int kofft_hip_pfb_synthesis_f32(kofft_hip_ctx *ctx, const float *spec, size_t rows, size_t frames, size_t bins, const float *g, size_t nh, size_t m,
                                size_t d, float scale, float *out, size_t out_first, size_t out_len)
{
    const int crc = pfb_synthesis_check(rows, frames, bins, nh, m, d, out_first, out_len, spec, g, out, ctx);
    if (crc || rows == 0 || frames == 0 || out_len == 0) return crc;
    return rows_host<float>(ctx, spec, out, rows, frames * bins * 2, out_len, g, nh, true, true,
                            [&](float *d_in, float *d_out, const float *d_g, size_t nb) {
                                return kofft_hip_dev_pfb_synthesis_f32(ctx, d_in, nb, frames, bins, d_g, nh, m, d, scale, d_out, out_first, out_len);
                            });
}

}  // extern "C"
