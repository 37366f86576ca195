// picture_impl.hip.h -- rows of audio to spectrogram pictures in one call: stft_magnitudes (visual/spectrogram.rs:52-76)
// -> the maximum -> color_from_magnitude_* per bin, f32 only like the reference.  No arithmetic is new: the magnitudes are the
// magnitudes kernels', the per-value colour functions are spectrogram_impl.hip.h's, included and not copied.
//
// The magnitudes go through the context's scratch, whole frames of the flat index t = row * frames + frame at a time, and every
// chunk is rendered before the next is produced.  What is new here:
//  * StftMagRowsMaxOnlyIO: the magnitudes kernels with StftMagRowsIO's accumulator (largest sum of squares, one root at the end, a
//    commit per row) and NO store -- the first pass of the row maximum where the magnitudes do not fit one chunk.
//  * pic_row_max_kernel: the row maximum of magnitudes that are in scratch anyway (a caller's window, a composed window length).
//  * the running maximum (web-spectrogram's compute_frame: m starts at 1e-12f, `if mag > m { m = mag }` walking frames, then bins,
//    BEFORE the pixel is coloured).  The comparison never selects a NaN and the seed is none, so m is the exact maximum over
//    {1e-12f} and the non-NaN magnitudes of the inclusive prefix, whatever the order of evaluation: three kernels per chunk,
//      pic_frame_max_kernel   a wavefront per frame: fmax[i] = max(1e-12f, the frame's magnitudes);
//      pic_frame_scan_kernel  a workgroup per row of the chunk: fmax[i] becomes the maximum of the frames BEFORE i of its row
//                             (exclusive; from the row's carry, which a chunk that ends inside the row leaves for the next one);
//      pic_pixel_max_kernel   a wavefront per frame: pmax[i][o] = max(fmax[i], magnitudes [0, o] of the frame), 64 bins per step
//                             with the running value carried from step to step.
//    The per-pixel maximum is MATERIALISED as a second scratch array that the render reads per pixel.  Folded into the render it
//    would need a scan along bins in kernels whose lanes walk bins in tiles of 64 owned by different workgroups (layout 1) or in
//    groups of four pixels that straddle frames (layout 0); the render is VALU-bound at about 208 instructions per pixel (5.22), so
//    one more 4-byte load per pixel is the cheaper side, and the render kernels keep ONE shape for all three maximum modes.
//  * pic_flat_kernel / pic_image_kernel: spec_flat_kernel / spec_image_kernel for a WINDOW of a picture: the maximum per row of the
//    batch (or per pixel), a first column f0 and the picture's own pitch in layout 1, and the 4-channel pixel R, G, B, 255.
#pragma once

#include "spectrogram_impl.hip.h"

namespace kofft {

// StftMagRowsIO without the stores: what is left is the accumulator.  `mags` stays null and is never dereferenced (the descriptors
// made from it are never stored through).
struct StftMagRowsMaxOnlyIO : StftMagRowsIO {
    __device__ __forceinline__ void store_acc(size_t xf, int o, cpx<float> v, Acc &acc) const
    {
        if (o < n / 2) {
            const unsigned row = (unsigned)row_of(xf);
            if (row != acc.row) {
                if (acc.s > 0.0f) atomicMax(max_bits + acc.row, __builtin_bit_cast(unsigned, sqrtf(acc.s)));
                acc = Acc{0.0f, row};
            }
            acc.s = __builtin_fmaxf(acc.s, sumsq(v));
        }
    }
    // the persistent kernel's forms: the largest sum of squares of the kept registers, no roots, no stores
    template <int NK>
    __device__ __forceinline__ static float mags_of(const cpx<float> (&v)[NK], float (&m)[NK])
    {
        float hi = v[0].re * v[0].re + v[0].im * v[0].im;
        m[0] = 0.0f;
#pragma unroll
        for (int i = 1; i < NK; ++i) {
            hi = __builtin_fmaxf(hi, v[i].re * v[i].re + v[i].im * v[i].im);
            m[i] = 0.0f;
        }
        return hi;
    }
    __device__ __forceinline__ void store_d_mag(rsrc_t, int, int, float, int) const {}
};

namespace host {

constexpr float kPicSeed = 1e-12f;  // compute_frame's starting maximum (web-spectrogram/src/lib.rs)

// pixel formats: 0 = 8-bit RGB, 1 = 16-bit RGB, 2 = 8-bit RGBA
constexpr int pic_px(int fmt) { return fmt == 1 ? 6 : (fmt == 2 ? 4 : 3); }
constexpr int pic_row_stride(int fmt) { return pic_px(fmt) * (SPEC_TF / 4) + 1; }  // dwords: odd, as spec_row_stride

template <int FMT>
__device__ __forceinline__ void pic_store_bytes(unsigned char *o, uint32_t c)
{
    if (FMT == 2) {
        for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)((c >> (8 * ch)) & 255u);
        o[3] = 255;
    } else {
        spec_store_bytes<FMT == 1>(o, c);
    }
}
// four pixels as pic_px(FMT) dwords
template <int FMT>
__device__ __forceinline__ void pic_pack4(const uint32_t (&c)[4], uint32_t *w)
{
    if (FMT == 2) {
        for (int e = 0; e < 4; ++e) w[e] = c[e] | 0xff000000u;
    } else {
        spec_pack4<FMT == 1>(c, w);
    }
}

// every row's starting value (mode 1: the carry of the running maximum)
__global__ __launch_bounds__(256) void pic_fill_kernel(float *__restrict__ dst, const size_t count, const float value)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) dst[i] = value;
}

// the row maximum (`if mag > max` from +0: a NaN is never selected) of `count` magnitudes of frames t0 .. of the flat index, into
// max_bits[row] by atomicMax on the bit patterns; grid-stride in steps that keep a wavefront's 64 lanes together
__global__ __launch_bounds__(256) void pic_row_max_kernel(const float *__restrict__ mags, unsigned *__restrict__ max_bits, const size_t frames,
                                                          const size_t half, const size_t t0, const size_t count)
{
    const size_t step = (size_t)gridDim.x * 256;
    const size_t rounds = (count + step - 1) / step;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t k = 0; k < rounds; ++k, i += step) {
        const bool in = i < count;
        const float v = in ? mags[i] : 0.0f;
        const unsigned row = in ? (unsigned)((t0 + i / half) / frames) : 0u;
        row_max_commit(max_bits, row, v, false);
    }
}

// a wavefront per frame: fmax[i] = the maximum of {1e-12f} and frame i's non-NaN magnitudes
__global__ __launch_bounds__(256) void pic_frame_max_kernel(const float *__restrict__ mags, float *__restrict__ fmax, const size_t nt, const int half)
{
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nt) return;
    const float *row = mags + i * (size_t)half;
    float m = kPicSeed;
    for (int o = lane; o < half; o += 64) m = __builtin_fmaxf(m, row[o]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) fmax[i] = m;
}

// A workgroup per row that has frames in the chunk [t0, t0 + nt): those frames are [a, b) of the chunk.  fmax[a .. b) becomes the
// exclusive prefix maximum, seeded with the row's carry (a row that begins in this chunk: its carry is still the seed the fill
// kernel wrote), and the carry becomes the maximum over all of them.  Thread j owns a contiguous run; the runs' maxima are
// scanned in LDS by thread 0 .. 255 in order (256 values).
__global__ __launch_bounds__(256) void pic_frame_scan_kernel(float *__restrict__ fmax, float *__restrict__ carry, const size_t frames,
                                                             const size_t t0, const size_t nt)
{
    __shared__ float part[256];
    const size_t row = t0 / frames + blockIdx.x;
    const size_t lo = row * frames, hi = lo + frames;
    const size_t a = (lo > t0 ? lo : t0) - t0, b = (hi < t0 + nt ? hi : t0 + nt) - t0;
    const size_t cnt = b - a, per = (cnt + 255) / 256;
    const size_t j0 = a + per * threadIdx.x < b ? a + per * threadIdx.x : b, j1 = j0 + per < b ? j0 + per : b;
    float m = kPicSeed;
    for (size_t j = j0; j < j1; ++j) m = __builtin_fmaxf(m, fmax[j]);
    part[threadIdx.x] = m;
    __syncthreads();
    const float c0 = carry[row];
    __syncthreads();  // (every thread has read the carry before thread 255 replaces it)
    float before = c0;
    for (int k = 0; k < (int)threadIdx.x; ++k) before = __builtin_fmaxf(before, part[k]);
    for (size_t j = j0; j < j1; ++j) {
        const float v = fmax[j];
        fmax[j] = before;
        before = __builtin_fmaxf(before, v);
    }
    if (threadIdx.x == 255) carry[row] = __builtin_fmaxf(before, part[255]);
}

// a wavefront per frame: pmax[i][o] = max(fmax[i], magnitudes [0, o] of frame i), NaNs skipped
__global__ __launch_bounds__(256) void pic_pixel_max_kernel(const float *__restrict__ mags, const float *__restrict__ fmax,
                                                            float *__restrict__ pmax, const size_t nt, const int half)
{
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nt) return;
    const float *row = mags + i * (size_t)half;
    float *dst = pmax + i * (size_t)half;
    float run = fmax[i];
    for (int o0 = 0; o0 < half; o0 += 64) {
        const int o = o0 + lane;
        float v = __builtin_fmaxf(run, o < half ? row[o] : 0.0f);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float up = __shfl_up(v, off);
            if (lane >= off) v = __builtin_fmaxf(v, up);
        }
        if (o < half) dst[o] = v;
        run = __shfl(v, 63);
    }
}

// ---- the render of a window of the batch's pictures ---------------------------------------------------------------------------
// Layout 0: frame t of the flat index is `bins` pixels at out + t * bins * PX, rows of the batch back to back, so a chunk of nt frames
// is ONE run of pixels; only the maximum knows about rows (row_max[row0 + (off + j) / row_px] for pixel j of the chunk, row_px the pixels
// of one picture and `off` the chunk's first pixel inside picture row0) or pixels (PMAX: pmax[j]).  `out` is the chunk's first byte.
// As spec_flat_kernel: a lane owns four consecutive pixels, and a chunk inside one row with a linear scale divides nothing.
template <int FMT, bool PMAX>
__global__ __launch_bounds__(256) void pic_flat_kernel(const float *__restrict__ mags, const float *__restrict__ pmax, unsigned char *__restrict__ out,
                                                       const size_t nt, const int bins, const float *__restrict__ row_max, const size_t row0,
                                                       const size_t off, const size_t row_px, const int mode, const float level, const int cmap,
                                                       const uint32_t *__restrict__ start)
{
    constexpr int PX = pic_px(FMT), NW = pic_px(FMT);
    const size_t total = nt * (size_t)bins, groups = (total + 3) / 4, step = (size_t)gridDim.x * 256;
    const bool vec_in = !start && (reinterpret_cast<size_t>(mags) & 15) == 0 && (!PMAX || (reinterpret_cast<size_t>(pmax) & 15) == 0);
    const bool vec_out = (reinterpret_cast<size_t>(out) & 3) == 0;
    const bool one_row = off + total <= row_px;                 // the whole launch lies in picture row0
    const bool narrow = off + total < (size_t(1) << 32);        // (then row_px does too, where it is divided by)
    const float mx0 = PMAX ? 0.0f : row_max[row0];
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += step) {
        const size_t j0 = 4 * q;
        const int n = total - j0 < 4 ? (int)(total - j0) : 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mx[4] = {mx0, mx0, mx0, mx0};
        if (PMAX) {
            if (vec_in && n == 4) {
                const spec_f4 x = *reinterpret_cast<const spec_f4 *>(pmax + j0);
                mx[0] = x.x, mx[1] = x.y, mx[2] = x.z, mx[3] = x.w;
            } else {
                for (int e = 0; e < n; ++e) mx[e] = pmax[j0 + e];
            }
        } else if (!one_row) {
            const size_t a = off + j0;
            size_t r = narrow ? (size_t)((unsigned)a / (unsigned)row_px) : a / row_px;
            size_t rem = row_px - (a - r * row_px);  // pixels of this group's first picture from its first pixel on
            float cur = row_max[row0 + r];
            for (int e = 0; e < n; ++e) {
                while ((size_t)e >= rem) {
                    ++r, rem += row_px;
                    cur = row_max[row0 + r];
                }
                mx[e] = cur;
            }
        }
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
        for (int e = 0; e < n; ++e) c[e] = spec_color(v[e], mx[e], mode, level, cmap);
        unsigned char *o = out + j0 * PX;
        if (vec_out && n == 4) {
            uint32_t w[NW];
            pic_pack4<FMT>(c, w);
            for (int j = 0; j < NW; ++j) reinterpret_cast<uint32_t *>(o)[j] = w[j];
        } else {
            for (int e = 0; e < n; ++e) pic_store_bytes<FMT>(o + e * PX, c[e]);
        }
    }
}

// Layout 1: nr rows of the batch from row0, of each the frames [f0, f0 + nf) (nr > 1: f0 == 0 and nf == frames).  mags holds them
// dense, [nr][nf][bins]; picture r is [bins][frames][PX] at out0 + r * frames * bins * PX, and this launch writes columns f0 .. of
// it.  spec_image_kernel's tiles, over (bins) x (the nf frames) x (the nr rows); a tile row's run of up to 64 frames starts at the
// picture's column f0 + x0, wherever that is against a 4-byte boundary: head / body / tail are cut at the run's own address, so
// every byte of the window is written exactly once and no byte outside it.
template <int FMT, bool LDS_T, bool PMAX>
__global__ __launch_bounds__(SPEC_THREADS) void pic_image_kernel(const float *__restrict__ mags, const float *__restrict__ pmax,
                                                                 unsigned char *__restrict__ out0, const size_t row0, const size_t f0,
                                                                 const size_t nf, const size_t frames, const int bins,
                                                                 const float *__restrict__ row_max, const int mode, const float level,
                                                                 const int cmap, const uint32_t *__restrict__ start, const unsigned tiles_b,
                                                                 const unsigned tiles_f)
{
    constexpr int PX = pic_px(FMT), NW = pic_px(FMT), STRIDE = pic_row_stride(FMT);
    __shared__ uint32_t tile[LDS_T ? SPEC_TB * STRIDE : 1];
    const unsigned per_row = tiles_b * tiles_f;
    const size_t j = blockIdx.x / per_row;  // row of this launch
    const unsigned tix = blockIdx.x - (unsigned)j * per_row;
    const float *m = mags + j * nf * (size_t)bins;
    const float *pm = PMAX ? pmax + j * nf * (size_t)bins : nullptr;
    unsigned char *out = out0 + (row0 + j) * frames * (size_t)bins * PX;
    const float mx_row = PMAX ? 0.0f : row_max[row0 + j];
    const int b0 = (int)(tix % tiles_b) * SPEC_TB;
    const size_t x0 = (size_t)(tix / tiles_b) * SPEC_TF;  // first frame of the tile, counted from f0
    const int nbv = bins - b0 < SPEC_TB ? bins - b0 : SPEC_TB;
    const int nfv = nf - x0 < (size_t)SPEC_TF ? (int)(nf - x0) : SPEC_TF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    if (lane < nbv) {
        const size_t img_row = (size_t)(bins - 1 - (b0 + lane));
        for (int q = wave; q < SPEC_TF / 4 && 4 * q < nfv; q += SPEC_THREADS / 64) {
            uint32_t c[4] = {0, 0, 0, 0};
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < nfv) {
                    const size_t x = x0 + 4 * q + e;
                    const float mx = PMAX ? pm[x * (size_t)bins + b0 + lane] : mx_row;
                    c[e] = spec_color(spec_value(m, start, x, b0 + lane, bins), mx, mode, level, cmap);
                }
            if (LDS_T) {
                uint32_t w[NW];
                pic_pack4<FMT>(c, w);
                for (int k = 0; k < NW; ++k) tile[lane * STRIDE + q * NW + k] = w[k];
            } else {
                unsigned char *o = out + (img_row * frames + f0 + x0 + 4 * q) * PX;
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < nfv) pic_store_bytes<FMT>(o + e * PX, c[e]);
            }
        }
    }
    if (!LDS_T) return;
    __syncthreads();
    const int nb = nfv * PX;
    for (int r = wave; r < nbv; r += SPEC_THREADS / 64) {
        const uint32_t *row = tile + r * STRIDE;
        unsigned char *g = out + ((size_t)(bins - 1 - (b0 + r)) * frames + f0 + x0) * PX;
        int head = (int)((4 - (reinterpret_cast<size_t>(g) & 3)) & 3);
        if (head > nb) head = nb;
        const int nd = (nb - head) / 4, tail = nb - head - 4 * nd;
        const int sh = 8 * head;
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
