// spectrogram_impl.hip.h -- the colour helpers of visual/spectrogram.rs:96-234 on device pointers, f32 only like the reference:
// magnitude_to_db, db_scale, map_color_u8 / _u16, color_from_magnitude_*, log_scale_bins (include/kofft_hip.h: the arithmetic
// contract).  Every operation is the reference's f32 operation in its order, one rounding each, nothing fused; log10 is the libm
// crate's log10f (libm_log10f.hip.h); the divisions are the correctly rounded ones.
//
// The per-value functions below are __host__ __device__: kofft_hip_map_color_u8 runs the same text on the host.
//
// Kernels:
//  * spec_db_kernel: magnitude_to_db or db_scale of `count` values, grid-stride, max_mag read from a pointer by every lane (one
//    scalar load).
//  * spec_flat_kernel<D16>: the frame-major picture [frames][bins][3].  Pixels are consecutive in memory, so a lane owns four of
//    them: one 16-byte load where the scale is linear and the input is aligned, four colours, three (D16: six) dword stores where
//    the output is 4-byte aligned, bytes otherwise and in the last, partial group.
//  * spec_image_kernel<D16, LDS_T>: the picture as an image [bins][frames][3], bin b of frame x at row bins - 1 - b, column x -- a
//    transpose of 3-byte (6-byte) pixels.  A workgroup of 256 owns a tile of 64 bins x 64 frames.  A lane loads along bins
//    (coalesced: lane = bin) and colours four consecutive frames of its bin in registers.
//      LDS_T = true: the 12 (24) bytes go to the lane's row of an LDS tile as dwords (row stride 49 / 97 dwords: odd, the 32 lanes
//      of a half write 32 banks); after the barrier a wavefront takes a row, whose run of up to 64 frames is one stretch of up to
//      192 (384) bytes of the picture: the bytes up to the first 4-byte boundary and after the last leave as single bytes, the body
//      as whole dwords, lane l the l-th, put together from two LDS dwords (the row's phase against the picture is one shift for the
//      whole row).  Tiles partition the picture, a tile's rows partition the tile, head / body / tail partition a row: each byte is
//      written exactly once.
//      LDS_T = false (kofft_hip_set_spectrogram_transpose(ctx, 0)): every lane stores its own 12 (24) bytes, one at a time.
//    The log scale replaces a lane's magnitude by the mean of its pixel's bins [start[p], start[p + 1]) (the host's ranges of the
//    caller's table), summed in increasing bin order from +0 and divided once; a pixel without bins is +0.
#pragma once

#include "host_common.hip.h"
#include "libm_log10f.hip.h"

namespace kofft {
namespace host {

constexpr int SPEC_TB = 64;        // bins per tile: one per lane
constexpr int SPEC_TF = 64;        // frames per tile
constexpr int SPEC_THREADS = 256;  // four wavefronts: 16 groups of four frames, four per wavefront
constexpr int spec_row_stride(bool d16) { return (d16 ? 6 : 3) * (SPEC_TF / 4) + 1; }  // dwords: 49 / 97

// f32::max: a NaN loses; of two equal values the second (the reference's floor) is returned
__host__ __device__ __forceinline__ float spec_max(float a, float b)
{
    if (a != a) return b;
    if (b != b) return a;
    return a > b ? a : b;
}
// f32::clamp(0.0, 1.0): a NaN stays, and so does -0
__host__ __device__ __forceinline__ float spec_clamp01(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }
// `as u8`: truncating, saturating, NaN -> 0
__host__ __device__ __forceinline__ uint32_t spec_u8(float v)
{
    if (!(v > 0.0f)) return 0;
    if (v >= 255.0f) return 255;
    return (uint32_t)(int)v;
}
// f32::round: half away from zero (exact for |v| < 2^23: v - trunc(v) is)
__host__ __device__ __forceinline__ float spec_round(float v)
{
    const float r = __builtin_truncf(v);
    const float d = v - r;
    if (d >= 0.5f) return r + 1.0f;
    if (d <= -0.5f) return r - 1.0f;
    return r;
}

// spectrogram.rs:96-102
__host__ __device__ __forceinline__ float spec_magnitude_to_db(float mag, float max_mag, float floor_db)
{
    if (max_mag <= 0.0f || mag <= 0.0f) return floor_db;
    const float db = 20.0f * libm_log10f(mag / max_mag);
    return spec_max(db, floor_db);
}
// spectrogram.rs:107-110
__host__ __device__ __forceinline__ float spec_db_scale(float mag, float max_mag, float dynamic_range)
{
    const float db = 20.0f * libm_log10f(spec_max(mag / max_mag, 1e-10f));
    return spec_clamp01((db + dynamic_range) / dynamic_range);
}

// lerp_u8 (spectrogram.rs:162-164) on the three channels of two stops; a colour is r | g << 8 | b << 16
__host__ __device__ __forceinline__ uint32_t spec_lerp3(uint32_t c0, uint32_t c1, float local)
{
    uint32_t out = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const float a = (float)((c0 >> (8 * ch)) & 255u), b = (float)((c1 >> (8 * ch)) & 255u);
        out |= spec_u8(a + (b - a) * local) << (8 * ch);
    }
    return out;
}
constexpr uint32_t spec_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }

// map_color_u8 (spectrogram.rs:113-187) for Fire 0, Legacy 1, Gray 2, Rainbow 6 (the host has refused the others)
__host__ __device__ __forceinline__ uint32_t spec_map_color(float t, int cmap)
{
    t = spec_clamp01(t);
    if (cmap == 0) {
        // the first window [s, e] with t >= s && t <= e; none (a NaN): the last one
        int i = 3;
        if (t >= 0.0f && t <= 0.25f) i = 0;
        else if (t >= 0.25f && t <= 0.5f) i = 1;
        else if (t >= 0.5f && t <= 0.75f) i = 2;
        float s, e;
        uint32_t c0, c1;
        switch (i) {
        case 0: s = 0.0f, e = 0.25f, c0 = spec_rgb(0, 0, 0), c1 = spec_rgb(128, 0, 128); break;
        case 1: s = 0.25f, e = 0.5f, c0 = spec_rgb(128, 0, 128), c1 = spec_rgb(255, 165, 0); break;
        case 2: s = 0.5f, e = 0.75f, c0 = spec_rgb(255, 165, 0), c1 = spec_rgb(255, 255, 0); break;
        default: s = 0.75f, e = 1.0f, c0 = spec_rgb(255, 255, 0), c1 = spec_rgb(255, 255, 255); break;
        }
        return spec_lerp3(c0, c1, (t - s) / (e - s));
    }
    if (cmap == 1) {
        const float r = 64.0f * (1.0f - t) + 255.0f * t;
        const float g = 255.0f * t;
        const float b = 64.0f * (1.0f - t) + 224.0f * t;
        return spec_u8(r) | spec_u8(g) << 8 | spec_u8(b) << 16;
    }
    if (cmap == 2) {
        const uint32_t g = spec_u8(spec_round(t * 255.0f));
        return g | g << 8 | g << 16;
    }
    // Rainbow: the strict `t >` walk over the stops; after the clamp it ends at the last segment at the latest
    const int i = (t > 0.25f ? 1 : 0) + (t > 0.5f ? 1 : 0) + (t > 0.75f ? 1 : 0) + (t > 0.9f ? 1 : 0);
    float s, e;
    uint32_t c0, c1;
    switch (i) {
    case 0: s = 0.0f, e = 0.25f, c0 = spec_rgb(0, 0, 0), c1 = spec_rgb(0, 0, 255); break;
    case 1: s = 0.25f, e = 0.5f, c0 = spec_rgb(0, 0, 255), c1 = spec_rgb(0, 255, 255); break;
    case 2: s = 0.5f, e = 0.75f, c0 = spec_rgb(0, 255, 255), c1 = spec_rgb(255, 255, 0); break;
    case 3: s = 0.75f, e = 0.9f, c0 = spec_rgb(255, 255, 0), c1 = spec_rgb(255, 0, 0); break;
    default: s = 0.9f, e = 1.0f, c0 = spec_rgb(255, 0, 0), c1 = spec_rgb(255, 255, 255); break;
    }
    return spec_lerp3(c0, c1, (t - s) / (e - s));  // (t1 > t0 in every segment)
}

// mode 0: color_from_magnitude_u8 (spectrogram.rs:196-200); mode 1: map_color_u8(db_scale(..))
__host__ __device__ __forceinline__ uint32_t spec_color(float mag, float max_mag, int mode, float level, int cmap)
{
    float t;
    if (mode == 0) {
        const float db = spec_magnitude_to_db(mag, max_mag, level);
        t = (db - level) / -level;
    } else {
        t = spec_db_scale(mag, max_mag, level);
    }
    return spec_map_color(t, cmap);
}

// which == 0: magnitude_to_db, else db_scale (internal linkage: picture_impl.hip.h includes this header into a second unit)
static __global__ __launch_bounds__(256) void spec_db_kernel(const float *__restrict__ mags, float *__restrict__ out, const size_t count,
                                                      const float *__restrict__ max_mag, const float level, const int which)
{
    const float mx = *max_mag;
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step)
        out[i] = which == 0 ? spec_magnitude_to_db(mags[i], mx, level) : spec_db_scale(mags[i], mx, level);
}

// the value pixel p of frame f is coloured from: its magnitude, or (start != nullptr) log_scale_bins' mean (spectrogram.rs:220-234)
__device__ __forceinline__ float spec_value(const float *__restrict__ mags, const uint32_t *__restrict__ start, size_t f, int p, int bins)
{
    const float *row = mags + f * (size_t)bins;
    if (!start) return row[p];
    const uint32_t k0 = start[p], k1 = start[p + 1];
    float sum = 0.0f;
    for (uint32_t k = k0; k < k1; ++k) sum += row[k];
    if (k1 > k0) sum = sum / (float)(k1 - k0);
    return sum;
}

// the bytes of one pixel, one store each
template <bool D16>
__device__ __forceinline__ void spec_store_bytes(unsigned char *o, uint32_t c)
{
    for (int ch = 0; ch < 3; ++ch) {
        const uint32_t v = (c >> (8 * ch)) & 255u;
        if (D16) {
            o[2 * ch] = (unsigned char)v;  // v * 257 = v << 8 | v, in the device's (little-endian) byte order
            o[2 * ch + 1] = (unsigned char)v;
        } else {
            o[ch] = (unsigned char)v;
        }
    }
}
// four pixels as 3 (D16: 6) dwords
template <bool D16>
__device__ __forceinline__ void spec_pack4(const uint32_t (&c)[4], uint32_t *w)
{
    if (D16) {
        uint32_t h[12];
        for (int e = 0; e < 4; ++e)
            for (int ch = 0; ch < 3; ++ch) h[3 * e + ch] = ((c[e] >> (8 * ch)) & 255u) * 257u;
        for (int j = 0; j < 6; ++j) w[j] = h[2 * j] | h[2 * j + 1] << 16;
    } else {
        w[0] = c[0] | c[1] << 24;
        w[1] = c[1] >> 8 | c[2] << 16;
        w[2] = c[2] >> 16 | c[3] << 8;
    }
}

typedef float spec_f4 __attribute__((ext_vector_type(4)));

template <bool D16>
__global__ __launch_bounds__(256) void spec_flat_kernel(const float *__restrict__ mags, unsigned char *__restrict__ out, const size_t frames,
                                                        const int bins, const float *__restrict__ max_mag, const int mode, const float level,
                                                        const int cmap, const uint32_t *__restrict__ start)
{
    constexpr int PX = D16 ? 6 : 3, NW = D16 ? 6 : 3;
    const float mx = *max_mag;
    const size_t total = frames * (size_t)bins, groups = (total + 3) / 4, step = (size_t)gridDim.x * 256;
    const bool vec_in = !start && (reinterpret_cast<size_t>(mags) & 15) == 0;
    const bool vec_out = (reinterpret_cast<size_t>(out) & 3) == 0;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += step) {
        const size_t j0 = 4 * q;
        const int n = total - j0 < 4 ? (int)(total - j0) : 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec_in && n == 4) {
            const spec_f4 x = *reinterpret_cast<const spec_f4 *>(mags + j0);
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        } else {
            size_t f = j0 / (size_t)bins;
            int p = (int)(j0 - f * (size_t)bins);
            for (int e = 0; e < n; ++e) {
                v[e] = spec_value(mags, start, f, p, bins);
                if (++p == bins) p = 0, ++f;
            }
        }
        uint32_t c[4] = {0, 0, 0, 0};
        for (int e = 0; e < n; ++e) c[e] = spec_color(v[e], mx, mode, level, cmap);
        unsigned char *o = out + j0 * PX;
        if (vec_out && n == 4) {
            uint32_t w[NW];
            spec_pack4<D16>(c, w);
            for (int j = 0; j < NW; ++j) reinterpret_cast<uint32_t *>(o)[j] = w[j];
        } else {
            for (int e = 0; e < n; ++e) spec_store_bytes<D16>(o + e * PX, c[e]);
        }
    }
}

template <bool D16, bool LDS_T>
__global__ __launch_bounds__(SPEC_THREADS) void spec_image_kernel(const float *__restrict__ mags, unsigned char *__restrict__ out,
                                                                  const size_t frames, const int bins, const float *__restrict__ max_mag,
                                                                  const int mode, const float level, const int cmap,
                                                                  const uint32_t *__restrict__ start, const unsigned tiles_b)
{
    constexpr int PX = D16 ? 6 : 3, NW = D16 ? 6 : 3, STRIDE = spec_row_stride(D16);
    __shared__ uint32_t tile[LDS_T ? SPEC_TB * STRIDE : 1];
    const float mx = *max_mag;
    const int b0 = (int)(blockIdx.x % tiles_b) * SPEC_TB;
    const size_t x0 = (size_t)(blockIdx.x / tiles_b) * SPEC_TF;
    const int nbv = bins - b0 < SPEC_TB ? bins - b0 : SPEC_TB;                  // bins of this tile
    const int nfv = frames - x0 < (size_t)SPEC_TF ? (int)(frames - x0) : SPEC_TF;  // frames of this tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // lane = bin; this wavefront's groups of four frames
    if (lane < nbv) {
        const size_t img_row = (size_t)(bins - 1 - (b0 + lane));
        for (int q = wave; q < SPEC_TF / 4 && 4 * q < nfv; q += SPEC_THREADS / 64) {
            uint32_t c[4] = {0, 0, 0, 0};
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < nfv) c[e] = spec_color(spec_value(mags, start, x0 + 4 * q + e, b0 + lane, bins), mx, mode, level, cmap);
            if (LDS_T) {
                uint32_t w[NW];
                spec_pack4<D16>(c, w);
                for (int j = 0; j < NW; ++j) tile[lane * STRIDE + q * NW + j] = w[j];
            } else {
                unsigned char *o = out + (img_row * frames + x0 + 4 * q) * PX;
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < nfv) spec_store_bytes<D16>(o + e * PX, c[e]);
            }
        }
    }
    if (!LDS_T) return;
    __syncthreads();
    // a wavefront per row: nb bytes of the tile's row r go to the picture at g
    const int nb = nfv * PX;
    for (int r = wave; r < nbv; r += SPEC_THREADS / 64) {
        const uint32_t *row = tile + r * STRIDE;
        unsigned char *g = out + ((size_t)(bins - 1 - (b0 + r)) * frames + x0) * PX;
        int head = (int)((4 - (reinterpret_cast<size_t>(g) & 3)) & 3);
        if (head > nb) head = nb;
        const int nd = (nb - head) / 4, tail = nb - head - 4 * nd;
        const int sh = 8 * head;  // (head < 4; the body starts at byte `head` of the row)
        for (int d = lane; d < nd; d += 64) {
            const int o = head + 4 * d;
            const uint32_t lo = row[o >> 2];
            uint32_t val = lo;
            if (sh) val = lo >> sh | row[(o >> 2) + 1] << (32 - sh);
            *reinterpret_cast<uint32_t *>(g + o) = val;
        }
        if (lane < head) g[lane] = (unsigned char)(row[0] >> (8 * lane));
        if (lane < tail) {
            const int o = head + 4 * nd + lane;
            g[o] = (unsigned char)(row[o >> 2] >> (8 * (o & 3)));
        }
    }
}

}  // namespace host
}  // namespace kofft
