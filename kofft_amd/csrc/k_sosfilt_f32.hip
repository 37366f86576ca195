// k_sosfilt_f32.hip -- batched IIR filtering of float rows (sosfilt_impl.hip.h, sosfilt_plan.h): the two kernels'
// instances, the argument checks and the device-pointer entry point.
#include "sosfilt_impl.hip.h"
#include "host_stage.hip.h"

namespace kofft {
namespace host {

static_assert(kSosTile == KOFFT_HIP_SOSFILT_TILE, "include/kofft_hip.h names the tile");
static_assert(kSosGroup == KOFFT_HIP_SOSFILT_GROUP, "include/kofft_hip.h names the group");
static_assert(kSosGroup == 8, "sosfilt_launch dispatches 1 .. 8 sections");

// The argument checks alone, in the order of include/kofft_hip.h and before the context or a device is touched.  KOFFT_OK with
// rows == 0 or nx == 0: nothing to do.  host_sos: sos is host memory, so a0 can be read.
// scan_chunk: null for sosfilt; for sosfilt_scan the chunk, checked directly after the flags, and the bytes of its state scratch join
// the overflow checks.
static int sosfilt_check(size_t rows, size_t nx, size_t sections, unsigned flags, const void *x, const void *sos, const void *zi, const void *zf,
                  const void *out, const kofft_hip_ctx *ctx, bool host_sos, const size_t *scan_chunk = nullptr)
{
    if (rows == 0 || nx == 0) return KOFFT_OK;
    if (sections == 0) return KOFFT_ERR_EMPTY_INPUT;
    if (flags & ~(unsigned)KOFFT_HIP_SOSFILT_REVERSE) return KOFFT_ERR_INVALID_VALUE;
    size_t x_bytes = 0, z_bytes = 0, sos_bytes = 0;
    if (scan_chunk) {
        if (*scan_chunk == 0 || *scan_chunk % kSosTile != 0) return KOFFT_ERR_INVALID_VALUE;
        const size_t D = 2 * (sections < kSosGroup ? sections : kSosGroup);
        size_t st = 0;  // (rows * C + D) * D floats: sos_scan_state_floats
        if (__builtin_mul_overflow(rows, sos_scan_chunks(nx, *scan_chunk), &st) || __builtin_add_overflow(st, D, &st) ||
            __builtin_mul_overflow(st, D * sizeof(float), &st))
            return KOFFT_ERR_UNSUPPORTED;
    }
    if (__builtin_mul_overflow(rows, nx, &x_bytes) || __builtin_mul_overflow(x_bytes, sizeof(float), &x_bytes) ||
        __builtin_mul_overflow(rows, sections, &z_bytes) || __builtin_mul_overflow(z_bytes, 2 * sizeof(float), &z_bytes) ||
        __builtin_mul_overflow(sections, 6 * sizeof(float), &sos_bytes))
        return KOFFT_ERR_UNSUPPORTED;
    if (!ctx || !x || !sos || !out) return KOFFT_ERR_NULL;
    if (out != x && overlaps(out, x_bytes, x, x_bytes)) return KOFFT_ERR_INVALID_VALUE;
    if (zi && zf && zf != zi && overlaps(zf, z_bytes, zi, z_bytes)) return KOFFT_ERR_INVALID_VALUE;
    if (overlaps(out, x_bytes, sos, sos_bytes) || (zf && overlaps(zf, z_bytes, sos, sos_bytes)) || (zf && overlaps(zf, z_bytes, out, x_bytes)) ||
        (zf && overlaps(zf, z_bytes, x, x_bytes)) || (zi && overlaps(out, x_bytes, zi, z_bytes)))
        return KOFFT_ERR_INVALID_VALUE;
    if (host_sos)
        for (size_t s = 0; s < sections; ++s)
            if (!(static_cast<const float *>(sos)[6 * s + 3] == 1.0f)) return KOFFT_ERR_INVALID_VALUE;
    return KOFFT_OK;
}

template <int NS>
static void sosfilt_launch_ns(kofft_hip_ctx *ctx, bool tiled, const float *src, const float *d_sos, const float *d_zi, float *d_zf, float *d_out,
                              const SosShape &s)
{
    if (tiled) {
        const size_t want = sos_row_groups(s.rows), cap = (size_t)ctx->num_cus * 64;
        hipLaunchKernelGGL((sosfilt_tiled_kernel<NS, kSosPrefetch>), dim3((unsigned)(want < cap ? want : cap)), dim3(64), 0, ctx->stream, src, d_sos,
                           d_zi, d_zf, d_out, s);
    } else {
        const size_t want = (s.rows + kSosPlainThreads - 1) / kSosPlainThreads, cap = (size_t)ctx->num_cus * 64;
        hipLaunchKernelGGL(sosfilt_plain_kernel<NS>, dim3((unsigned)(want < cap ? want : cap)), dim3(kSosPlainThreads), 0, ctx->stream, src, d_sos,
                           d_zi, d_zf, d_out, s);
    }
}

// mode 2: the tiled kernel wherever it exists, which is everywhere; mode 1: the measured rule (sos_route); mode 0: never
static bool sosfilt_use_tiled(const kofft_hip_ctx *ctx, size_t rows) { return ctx->sosfilt_tiled == 2 || (ctx->sosfilt_tiled == 1 && sos_route(rows) == 1); }

}  // namespace host
}  // namespace kofft

using namespace kofft;
using namespace kofft::host;

extern "C" {

int kofft_hip_dev_sosfilt_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                              const float *d_zi, float *d_zf, unsigned flags, float *d_out)
{
    const int crc = sosfilt_check(rows, nx, sections, flags, d_x, d_sos, d_zi, d_zf, d_out, ctx, false);
    if (crc || rows == 0 || nx == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool tiled = sosfilt_use_tiled(ctx, rows);
    SosShape s{};
    s.rows = rows;
    s.nx = nx;
    s.sections = sections;
    s.reverse = (flags & KOFFT_HIP_SOSFILT_REVERSE) ? 1 : 0;
    const size_t passes = sos_passes(sections, kSosGroup);
    for (size_t p = 0; p < passes; ++p) {  // pass p filters what pass p - 1 left in `out`
        s.first = p * kSosGroup;
        const float *src = p == 0 ? d_x : d_out;
        switch (sos_pass_sections(p, sections, kSosGroup)) {
        case 1: sosfilt_launch_ns<1>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 2: sosfilt_launch_ns<2>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 3: sosfilt_launch_ns<3>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 4: sosfilt_launch_ns<4>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 5: sosfilt_launch_ns<5>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 6: sosfilt_launch_ns<6>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        case 7: sosfilt_launch_ns<7>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        default: sosfilt_launch_ns<8>(ctx, tiled, src, d_sos, d_zi, d_zf, d_out, s); break;
        }
        KOFFT_HIP_TRY(ctx, hipGetLastError());
    }
    return KOFFT_OK;
}

// up to four row arrays: x up, out down, zi up, zf down (an absent state is an empty array and reaches the device as null); the
// coefficients are the side input, uploaded once
int kofft_hip_sosfilt_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                          float *zf, unsigned flags, float *out)
{
    const int crc = sosfilt_check(rows, nx, sections, flags, x, sos, zi, zf, out, ctx, true);
    if (crc || rows == 0 || nx == 0) return crc;
    const HostArray<float> a[4] = {{x, nullptr, nx}, {nullptr, out, nx}, {zi, nullptr, zi ? 2 * sections : 0}, {nullptr, zf, zf ? 2 * sections : 0}};
    return rows_host_n<float>(ctx, rows, 4, a, sos, 6 * sections, true, true, [&](float *const *d, const float *d_sos, size_t nr) {
        return kofft_hip_dev_sosfilt_f32(ctx, d[0], nr, nx, d_sos, sections, zi ? d[2] : nullptr, zf ? d[3] : nullptr, flags, d[1]);
    });
}

int kofft_hip_sosfilt_route(size_t rows, int *route)
{
    if (!route) return KOFFT_ERR_NULL;
    *route = sos_route(rows);
    return KOFFT_OK;
}

int kofft_hip_set_sosfilt_tiled(kofft_hip_ctx *ctx, int on) { return set_route(ctx, &kofft_hip_ctx::sosfilt_tiled, on, 0, 2); }

}  // extern "C"

// ---- the scan along time ----
template <int NS>
static void sosfilt_scan_launch_ns(kofft_hip_ctx *ctx, const float *src, const float *d_sos, const float *d_zi, float *d_zf, float *d_out, float *st,
                                   const SosScanShape &s)
{
    constexpr unsigned D = 2 * NS;
    const size_t cap = (size_t)ctx->num_cus * 64;
    if (s.chunks > 1) {
        const size_t w1 = sos_row_groups(s.rows * (s.chunks - 1) + D), wc = (s.rows - 1) / (64 / D) + 1;
        hipLaunchKernelGGL((sosfilt_scan_walk_kernel<NS, false>), dim3((unsigned)(w1 < cap ? w1 : cap)), dim3(64), 0, ctx->stream, src, d_sos,
                           (const float *)nullptr, (float *)nullptr, (float *)nullptr, st, s);
        hipLaunchKernelGGL(sosfilt_scan_carry_kernel<NS>, dim3((unsigned)(wc < cap ? wc : cap)), dim3(64), 0, ctx->stream, st, d_zi, s);
    }
    const size_t w2 = sos_row_groups(s.rows * s.chunks);
    hipLaunchKernelGGL((sosfilt_scan_walk_kernel<NS, true>), dim3((unsigned)(w2 < cap ? w2 : cap)), dim3(64), 0, ctx->stream, src, d_sos, d_zi, d_zf,
                       d_out, st, s);
}

extern "C" {

int kofft_hip_dev_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                                   const float *d_zi, float *d_zf, size_t chunk, unsigned flags, float *d_out)
{
    const int crc = sosfilt_check(rows, nx, sections, flags, d_x, d_sos, d_zi, d_zf, d_out, ctx, false, &chunk);
    if (crc || rows == 0 || nx == 0) return crc;
    KOFFT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t C = sos_scan_chunks(nx, chunk), passes = sos_passes(sections, kSosGroup);
    const unsigned Dmax = 2 * sos_pass_sections(0, sections, kSosGroup);
    // the states of a batch beyond the scratch cap: pieces of whole rows, every pass of a piece before the next piece
    const size_t piece = scratch_chunk_rows(ctx->scratch_chunk_bytes, C > 1 ? C * Dmax * sizeof(float) : 0, rows);
    if (C > 1) {
        const int erc = ensure(ctx, ctx->real_tmp, sos_scan_state_floats(piece, C, Dmax) * sizeof(float));
        if (erc) return erc;
    }
    float *st = static_cast<float *>(ctx->real_tmp.p);
    return for_chunks(rows, piece, [&](size_t r0, size_t nr) {
        SosScanShape s{};
        s.rows = nr;
        s.nx = nx;
        s.sections = sections;
        s.chunk = chunk;
        s.chunks = C;
        s.reverse = (flags & KOFFT_HIP_SOSFILT_REVERSE) ? 1 : 0;
        const float *zi = d_zi ? d_zi + r0 * sections * 2 : nullptr;
        float *zf = d_zf ? d_zf + r0 * sections * 2 : nullptr, *o = d_out + r0 * nx;
        for (size_t p = 0; p < passes; ++p) {  // pass p filters what pass p - 1 left in `out`
            s.first = p * kSosGroup;
            const float *src = p == 0 ? d_x + r0 * nx : o;
            switch (sos_pass_sections(p, sections, kSosGroup)) {
            case 1: sosfilt_scan_launch_ns<1>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 2: sosfilt_scan_launch_ns<2>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 3: sosfilt_scan_launch_ns<3>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 4: sosfilt_scan_launch_ns<4>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 5: sosfilt_scan_launch_ns<5>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 6: sosfilt_scan_launch_ns<6>(ctx, src, d_sos, zi, zf, o, st, s); break;
            case 7: sosfilt_scan_launch_ns<7>(ctx, src, d_sos, zi, zf, o, st, s); break;
            default: sosfilt_scan_launch_ns<8>(ctx, src, d_sos, zi, zf, o, st, s); break;
            }
            KOFFT_HIP_TRY(ctx, hipGetLastError());
        }
        return (int)KOFFT_OK;
    });
}


// the same staging as kofft_hip_sosfilt_f32: rows are independent
int kofft_hip_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                               float *zf, size_t chunk, unsigned flags, float *out)
{
    const int crc = sosfilt_check(rows, nx, sections, flags, x, sos, zi, zf, out, ctx, true, &chunk);
    if (crc || rows == 0 || nx == 0) return crc;
    const HostArray<float> a[4] = {{x, nullptr, nx}, {nullptr, out, nx}, {zi, nullptr, zi ? 2 * sections : 0}, {nullptr, zf, zf ? 2 * sections : 0}};
    return rows_host_n<float>(ctx, rows, 4, a, sos, 6 * sections, true, true, [&](float *const *d, const float *d_sos, size_t nr) {
        return kofft_hip_dev_sosfilt_scan_f32(ctx, d[0], nr, nx, d_sos, sections, zi ? d[2] : nullptr, zf ? d[3] : nullptr, chunk, flags, d[1]);
    });
}

int kofft_hip_sosfilt_scan_chunk(size_t rows, size_t nx, size_t sections, size_t *chunk)
{
    if (!chunk) return KOFFT_ERR_NULL;
    *chunk = (size_t)sos_scan_chunk_rule(rows, nx, sections);
    return KOFFT_OK;
}

}  // extern "C"
