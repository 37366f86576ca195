// wavelet_impl.hip.h -- wavelet::* (wavelet.rs:12-117, 154-567) on device pointers, f32 only like the reference: haar, db2, db4, sym4
// and coif1, forward and inverse, single level and multi level.
//
// The arithmetic is the reference's, term for term (-ffp-contract=off: nothing is fused):
//  * forward, output i, j = 2i, r() the reference's `while` reflection over the input length (odd in a single-level call):
//      haar  (x[j] + x[j+1]) / 2.0 and (x[j] - x[j+1]) / 2.0, written * 0.5f (the same correctly rounded value: 0.5 is exact);
//      db2   h0 * r(j) + h1 * r(j+1) + h2 * r(j+2) + h3 * r(j+3), left to right, NOT seeded;
//      db4 / sym4 / coif1   acc = +0.0, then acc += h[k] * r(j+k) for k ascending (the same with g for the detail);
//  * inverse: haar out[2i] = a + d, out[2i+1] = a - d; the others start every output at +0.0 and add (g[k] * a[i] + h[k] * d[i])
//    to out[r(2i+k)] over (i, k) in lexicographic order.  Here every lane GATHERS one output: the direct hits of output p come from
//    i = p/2 - (L/2 - 1) .. p/2 in ascending i, one per i; the reflected hits land in the last L - 1 outputs (rows of at least L
//    samples), and those outputs -- and every output of a row shorter than L -- scan the (i, k) pairs that can reach them in the
//    reference's order (inv_out).
//  * multi level (wavelet.rs:54-84): an odd current row is padded with its last sample before each level; the pad is virtual here
//    (reads of index c return sample c - 1), the reflection runs over the padded length.
// Coefficients: taps(), one constexpr table for host and device, each literal the f32 nearest to the reference's decimal string
// (an `f` literal: rounding through f64 first can differ).  The inverse filters are the reference's own arrays (gk / hk for db2),
// never derived from the forward ones.
//
// Kernels:
//  * wavelet_fwd_kernel<W> / wavelet_inv_kernel<W>: one level, streaming.  A workgroup owns a tile of WV_TILE outputs of one row
//    (its samples plus the L - 2 halo staged in LDS, 16-byte loads where aligned) or, for short rows, WV_TILE / n whole rows;
//    outputs leave in groups of four, 16-byte stores where the address is aligned.  Outputs whose taps reflect read global memory.
//    The inverse stages approximations and details the same way (16-byte loads where aligned).
//  * wavelet_fwd_fused_kernel<W> / wavelet_inv_fused_kernel<W>: every level of one row, or of several short rows, with the rows kept
//    in LDS; each level's detail is written once, straight to its place in the packed output.  Rows of up to kWaveletFusedMax
//    samples (forward: the input; inverse: the output).
#pragma once

#include "host_common.hip.h"

#include <cstdint>

namespace kofft {
namespace wav {

enum : int { HAAR = 0, DB2 = 1, DB4 = 2, SYM4 = 3, COIF1 = 4, NFAM = 5 };

// lo multiplies the signal (forward) or the approximation (inverse); hi gives the detail (forward) or multiplies it (inverse)
struct Taps {
    int len;
    float lo[8];
    float hi[8];
};

__host__ __device__ constexpr Taps taps(int w, bool inverse)
{
    switch (w * 2 + (inverse ? 1 : 0)) {
    case DB2 * 2:  // wavelet.rs:159-166
        return Taps{4, {0.4829629131445341f, 0.8365163037378079f, 0.2241438680420134f, -0.1294095225512604f},
                    {-0.1294095225512604f, -0.2241438680420134f, 0.8365163037378079f, -0.4829629131445341f}};
    case DB2 * 2 + 1:  // gk / hk, wavelet.rs:225-242
        return Taps{4, {0.4829629131445341f, 0.8365163037378079f, 0.2241438680420134f, -0.1294095225512604f},
                    {-0.1294095225512604f, -0.2241438680420134f, 0.8365163037378079f, -0.4829629131445341f}};
    case DB4 * 2:  // wavelet.rs:268-287
        return Taps{8, {-0.010597401785069032f, 0.0328830116668852f, 0.030841381835560764f, -0.18703481171909309f,
                        -0.027983769416859854f, 0.6308807679298589f, 0.7148465705529157f, 0.2303778133088965f},
                    {-0.2303778133088965f, 0.7148465705529157f, -0.6308807679298589f, -0.027983769416859854f, 0.18703481171909309f,
                     0.030841381835560764f, -0.0328830116668852f, -0.010597401785069032f}};
    case DB4 * 2 + 1:  // wavelet.rs:316-335
        return Taps{8, {0.2303778133088965f, 0.7148465705529157f, 0.6308807679298589f, -0.027983769416859854f,
                        -0.18703481171909309f, 0.030841381835560764f, 0.0328830116668852f, -0.010597401785069032f},
                    {-0.010597401785069032f, -0.0328830116668852f, 0.030841381835560764f, 0.18703481171909309f,
                     -0.027983769416859854f, -0.6308807679298589f, 0.7148465705529157f, -0.2303778133088965f}};
    case SYM4 * 2:  // wavelet.rs:362-381
        return Taps{8, {-0.07576571478927333f, -0.02963552764599851f, 0.49761866763201545f, 0.8037387518059161f,
                        0.29785779560527736f, -0.09921954357684722f, -0.012603967262037833f, 0.0322231006040427f},
                    {-0.0322231006040427f, -0.012603967262037833f, 0.09921954357684722f, 0.29785779560527736f, -0.8037387518059161f,
                     0.49761866763201545f, 0.02963552764599851f, -0.07576571478927333f}};
    case SYM4 * 2 + 1:  // wavelet.rs:410-429
        return Taps{8, {0.0322231006040427f, -0.012603967262037833f, -0.09921954357684722f, 0.29785779560527736f,
                        0.8037387518059161f, 0.49761866763201545f, -0.02963552764599851f, -0.07576571478927333f},
                    {-0.07576571478927333f, 0.02963552764599851f, 0.49761866763201545f, -0.8037387518059161f, 0.29785779560527736f,
                     0.09921954357684722f, -0.012603967262037833f, -0.0322231006040427f}};
    case COIF1 * 2:  // wavelet.rs:456-471
        return Taps{6, {-0.015655728135791993f, -0.07273261951252645f, 0.3848648468648578f, 0.8525720202116004f, 0.3378976624574818f,
                        -0.07273261951252645f},
                    {0.07273261951252645f, 0.3378976624574818f, -0.8525720202116004f, 0.3848648468648578f, 0.07273261951252645f,
                     -0.015655728135791993f}};
    case COIF1 * 2 + 1:  // wavelet.rs:500-515
        return Taps{6, {-0.07273261951252645f, 0.3378976624574818f, 0.8525720202116004f, 0.3848648468648578f, -0.07273261951252645f,
                        -0.015655728135791993f},
                    {-0.015655728135791993f, 0.07273261951252645f, 0.3848648468648578f, -0.8525720202116004f, 0.3378976624574818f,
                     0.07273261951252645f}};
    default:  // haar: no coefficient arrays (wavelet.rs:12-33)
        return Taps{2, {}, {}};
    }
}

// the reference's reflection (wavelet.rs:168-178); every length it runs over is >= 2 (the guard keeps a bad call from spinning)
__host__ __device__ inline int reflect(int idx, int len)
{
    if (len < 2) return 0;
    while (idx < 0 || idx >= len) idx = idx < 0 ? -idx : 2 * (len - 1) - idx;
    return idx;
}

// forward output at j = 2i; get(idx) is sample idx of the (reflected) row
template <int W, class Get>
__device__ __forceinline__ void fwd_out(const Get &get, int j, float &a, float &d)
{
    constexpr Taps t = taps(W, false);
    if constexpr (W == HAAR) {
        const float x0 = get(j), x1 = get(j + 1);
        a = (x0 + x1) * 0.5f;
        d = (x0 - x1) * 0.5f;
    } else if constexpr (W == DB2) {
        const float x0 = get(j), x1 = get(j + 1), x2 = get(j + 2), x3 = get(j + 3);
        a = t.lo[0] * x0 + t.lo[1] * x1 + t.lo[2] * x2 + t.lo[3] * x3;
        d = t.hi[0] * x0 + t.hi[1] * x1 + t.hi[2] * x2 + t.hi[3] * x3;
    } else {
        float sa = 0.0f, sd = 0.0f;
#pragma unroll
        for (int k = 0; k < t.len; ++k) {
            const float v = get(j + k);
            sa = sa + t.lo[k] * v;
            sd = sd + t.hi[k] * v;
        }
        a = sa;
        d = sd;
    }
}

// inverse output p of a row of len = 2c outputs; ga(i) / gd(i) read the approximation / detail.  Direct-only outputs (all but
// the last L - 1 of a row of at least L) take their hits in ascending i; the rest scan every (i, k) that can reach them, in order.
template <int W, class GA, class GD>
__device__ __forceinline__ float inv_out(const GA &ga, const GD &gd, int p, int len, int c)
{
    constexpr Taps t = taps(W, true);
    constexpr int L = t.len, H = L / 2;
    if constexpr (W == HAAR) {
        const int i = p >> 1;
        const float a = ga(i), d = gd(i);
        return (p & 1) ? a - d : a + d;
    } else {
        float acc = 0.0f;
        if (len >= L && p + L - 1 < len) {
            const int m = p >> 1, par = p & 1;
#pragma unroll
            for (int s = 0; s < H; ++s) {
                const int i = m - (H - 1) + s;
                const int k0 = 2 * (H - 1 - s);  // k = k0 + par
                const float lo = par ? t.lo[k0 + 1] : t.lo[k0], hi = par ? t.hi[k0 + 1] : t.hi[k0];
                if (i >= 0) {
                    const float term = lo * ga(i) + hi * gd(i);
                    acc = acc + term;
                }
            }
        } else {
            for (int i = len >= 2 * L ? (len - 2 * L) / 2 : 0; i < c; ++i) {
#pragma unroll
                for (int k = 0; k < L; ++k) {
                    if (reflect(2 * i + k, len) == p) {
                        const float term = t.lo[k] * ga(i) + t.hi[k] * gd(i);
                        acc = acc + term;
                    }
                }
            }
        }
        return acc;
    }
}

typedef unsigned wv_u4 __attribute__((ext_vector_type(4)));

// v[first .. last) to p[first .. last): one 16-byte store (guarded) when all four go and p is 16-byte aligned
__device__ __forceinline__ void store4(float *p, const float (&v)[4], int first, int last)
{
    if (first == 0 && last == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const wv_u4 bits = {__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]), __builtin_bit_cast(unsigned, v[2]),
                            __builtin_bit_cast(unsigned, v[3])};
        *reinterpret_cast<wv_u4 *>(p) = bits;
        b128_store_guard(bits);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q >= first && q < last) p[q] = v[q];
}

// elements before p's next 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int misalign(const float *p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// g[0 .. cnt) -> s[0 .. cnt): 16-byte loads from the first 16-byte boundary of g on, 4-byte loads for the ends
__device__ __forceinline__ void stage(const float *__restrict__ g, float *s, int cnt, int tid, int nthr)
{
    int head = (4 - misalign(g)) & 3;
    if (head > cnt) head = cnt;
    if (tid < head) s[tid] = g[tid];
    const int nv = (cnt - head) >> 2;
    const float4 *gv = reinterpret_cast<const float4 *>(g + head);
    for (int q = tid; q < nv; q += nthr) {
        const float4 v = gv[q];
        const int e = head + 4 * q;
        s[e] = v.x;
        s[e + 1] = v.y;
        s[e + 2] = v.z;
        s[e + 3] = v.w;
    }
    for (int e = head + 4 * nv + tid; e < cnt; e += nthr) s[e] = g[e];
}

constexpr int WV_BLOCK = 256;
constexpr int WV_TILE = 1024;               // forward outputs per workgroup (four per lane); the inverse takes 2 * WV_TILE
constexpr int WV_FWD_LDS = 3 * WV_TILE + 8;  // packed rows: (WV_TILE / n) * (2n + 1) <= 3 * WV_TILE samples; a tile: 2 * WV_TILE + L - 2
constexpr int WV_INV_LDS = WV_TILE + 8;     // packed rows: WV_TILE / c * c; a tile: WV_TILE + 4 (H - 1 <= 3 entries before it)
constexpr int WF_BLOCK = 512;

// ---- one level, streaming ---------------------------------------------------------------------------------------------------------
// Rows of c samples (stride c), reflected over lp (= c, or c + 1 for a padded level), n = lp / 2 outputs each (stride n).  rpt > 1:
// every workgroup takes rpt whole rows (n <= WV_TILE / 2); rpt == 1: blockIdx.x is the tile of WV_TILE outputs.  blockIdx.y strides
// over the row groups.
template <int W>
__global__ __launch_bounds__(WV_BLOCK) void wavelet_fwd_kernel(const float *__restrict__ x, float *__restrict__ a, float *__restrict__ d,
                                                              const int c, const int lp, const size_t rows, const int rpt)
{
    __shared__ float s[WV_FWD_LDS];
    constexpr int L = taps(W, false).len;
    const int n = lp >> 1;
    const int i0 = rpt > 1 ? 0 : (int)blockIdx.x * WV_TILE;
    const int ni = rpt > 1 ? n : (n - i0 < WV_TILE ? n - i0 : WV_TILE);
    for (size_t g = blockIdx.y; g * rpt < rows; g += gridDim.y) {
        const size_t r0 = g * rpt;
        const int nr = rows - r0 < (size_t)rpt ? (int)(rows - r0) : rpt;
        const int cnt = rpt > 1 ? nr * c : (2 * ni + L - 2 < c - 2 * i0 ? 2 * ni + L - 2 : c - 2 * i0);
        stage(x + r0 * c + 2 * i0, s, cnt, threadIdx.x, WV_BLOCK);
        __syncthreads();
        const int total = nr * ni;
        float *ag = a + r0 * n + i0, *dg = d + r0 * n + i0;
        const int s0 = misalign(ag);
        for (int grp = threadIdx.x; 4 * grp < total + s0; grp += WV_BLOCK) {
            const int lo = 4 * grp - s0;
            const int first = lo < 0 ? -lo : 0, last = total - lo < 4 ? total - lo : 4;
            int r = (lo + first) / ni, li = lo + first - r * ni;
            float va[4] = {0.f, 0.f, 0.f, 0.f}, vd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < first || q >= last) continue;
                const int j = 2 * (i0 + li);
                if (j + L - 1 < c) {
                    const float *sr = s + r * c - 2 * i0;
                    fwd_out<W>([&](int idx) { return sr[idx]; }, j, va[q], vd[q]);
                } else {
                    const float *row = x + (r0 + r) * c;
                    fwd_out<W>([&](int idx) { int e = reflect(idx, lp); return row[e < c ? e : c - 1]; }, j, va[q], vd[q]);
                }
                if (++li == ni) {
                    li = 0;
                    ++r;
                }
            }
            store4(ag + lo, va, first, last);
            store4(dg + lo, vd, first, last);
        }
        __syncthreads();
    }
}

// Rows of c approximations (stride c) and details (stride ds >= c) to rows of 2c outputs.  rpt > 1: rpt whole rows per workgroup
// (c <= WV_TILE / 2); rpt == 1: blockIdx.x is the tile of 2 * WV_TILE outputs.
template <int W>
__global__ __launch_bounds__(WV_BLOCK) void wavelet_inv_kernel(const float *__restrict__ a, const float *__restrict__ d, float *__restrict__ out,
                                                              const int c, const int ds, const size_t rows, const int rpt)
{
    __shared__ float sa[WV_INV_LDS], sd[WV_INV_LDS];
    const int len = 2 * c;
    const int i0 = rpt > 1 ? 0 : (int)blockIdx.x * WV_TILE;
    const int base = rpt > 1 ? 0 : i0 - 4;  // LDS entry e of row r holds index base + e
    const int ilo = base > 0 ? base : 0, ihi = rpt > 1 ? c : (i0 + WV_TILE < c ? i0 + WV_TILE : c);
    const int np = rpt > 1 ? len : (len - 2 * i0 < 2 * WV_TILE ? len - 2 * i0 : 2 * WV_TILE);
    for (size_t g = blockIdx.y; g * rpt < rows; g += gridDim.y) {
        const size_t r0 = g * rpt;
        const int nr = rows - r0 < (size_t)rpt ? (int)(rows - r0) : rpt;
        // the staged entries of the approximations are one contiguous span (a tile of one row, or whole rows of c); so are the
        // details' unless their rows are longer than c (extra entries a multi-level inverse ignores): 4-byte loads then
        const int per = ihi - ilo, span = (nr - 1) * c + per;
        stage(a + r0 * c + ilo, sa + ilo - base, span, threadIdx.x, WV_BLOCK);
        if (ds == c || nr == 1) {
            stage(d + r0 * ds + ilo, sd + ilo - base, span, threadIdx.x, WV_BLOCK);
        } else {
            for (int e = threadIdx.x; e < nr * per; e += WV_BLOCK) {
                const int r = e / per, i = ilo + e - r * per;
                sd[r * c + i - base] = d[(r0 + r) * ds + i];
            }
        }
        __syncthreads();
        const int total = nr * np;
        float *og = out + r0 * len + 2 * i0;
        const int s0 = misalign(og);
        for (int grp = threadIdx.x; 4 * grp < total + s0; grp += WV_BLOCK) {
            const int lo = 4 * grp - s0;
            const int first = lo < 0 ? -lo : 0, last = total - lo < 4 ? total - lo : 4;
            int r = (lo + first) / np, lp = lo + first - r * np;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < first || q >= last) continue;
                const int p = 2 * i0 + lp;
                if (W == HAAR || p + taps(W, true).len - 1 < len) {  // every hit inside the staged entries
                    const float *ra = sa + r * c - base, *rd = sd + r * c - base;
                    v[q] = inv_out<W>([&](int i) { return ra[i]; }, [&](int i) { return rd[i]; }, p, len, c);
                } else {
                    const float *ra = a + (r0 + r) * c, *rd = d + (r0 + r) * ds;
                    v[q] = inv_out<W>([&](int i) { return ra[i]; }, [&](int i) { return rd[i]; }, p, len, c);
                }
                if (++lp == np) {
                    lp = 0;
                    ++r;
                }
            }
            store4(og + lo, v, first, last);
        }
        __syncthreads();
    }
}

// ---- every level in LDS -------------------------------------------------------------------------------------------------------------
// rpb rows of len samples per workgroup (row0 + blockIdx.x * rpb on; rows are contiguous, so are their outputs).  LDS: [bufa | rpb * ceil(len / 2)],
// the levels ping-pong between the two.  det: the packed details, level l at sum_{m < l} rows * a_m, rows of a_l.
template <int W>
__global__ __launch_bounds__(WF_BLOCK) void wavelet_fwd_fused_kernel(const float *__restrict__ x, float *__restrict__ approx, float *__restrict__ det,
                                                                    const int len, const int levels, const size_t rows, const size_t row0, const int rpb,
                                                                    const int bufa)
{
    extern __shared__ float sm[];
    constexpr int L = taps(W, false).len;
    const size_t r0 = row0 + (size_t)blockIdx.x * rpb;
    const int nr = rows - r0 < (size_t)rpb ? (int)(rows - r0) : rpb;
    stage(x + r0 * len, sm, nr * len, threadIdx.x, WF_BLOCK);
    __syncthreads();
    float *src = sm, *dst = sm + bufa;
    int c = len;
    size_t off = 0;
    for (int l = 0; l < levels; ++l) {
        const int lp = c + (c & 1), n = lp >> 1, total = nr * n;
        float *dg = det + off + r0 * n;
        const int s0 = misalign(dg);
        for (int grp = threadIdx.x; 4 * grp < total + s0; grp += WF_BLOCK) {
            const int lo = 4 * grp - s0;
            const int first = lo < 0 ? -lo : 0, last = total - lo < 4 ? total - lo : 4;
            int r = (lo + first) / n, i = lo + first - r * n;
            float va[4] = {0.f, 0.f, 0.f, 0.f}, vd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < first || q >= last) continue;
                const float *sr = src + r * c;
                const int j = 2 * i;
                if (j + L - 1 < c) fwd_out<W>([&](int idx) { return sr[idx]; }, j, va[q], vd[q]);
                else fwd_out<W>([&](int idx) { int e = reflect(idx, lp); return sr[e < c ? e : c - 1]; }, j, va[q], vd[q]);
                dst[lo + q] = va[q];
                if (++i == n) {
                    i = 0;
                    ++r;
                }
            }
            store4(dg + lo, vd, first, last);
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
        c = n;
        off += rows * (size_t)n;
    }
    float *ag = approx + r0 * c;
    const int total = nr * c, s0 = misalign(ag);
    for (int grp = threadIdx.x; 4 * grp < total + s0; grp += WF_BLOCK) {
        const int lo = 4 * grp - s0;
        const int first = lo < 0 ? -lo : 0, last = total - lo < 4 ? total - lo : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q >= first && q < last) v[q] = src[lo + q];
        store4(ag + lo, v, first, last);
    }
}

constexpr int kMaxLevels = 64;
struct Lens {
    int v[kMaxLevels];
};

// rpb rows of n approximations per workgroup, details dl.v[l] long (finest first, packed as in the forward), outputs n << levels
// long.  LDS: two buffers of bufh floats (rpb * (n << (levels - 1)), the longest intermediate); the last level writes global memory.
template <int W>
__global__ __launch_bounds__(WF_BLOCK) void wavelet_inv_fused_kernel(const float *__restrict__ approx, const float *__restrict__ det, float *__restrict__ out,
                                                                    const int n, const int levels, const size_t rows, const size_t row0, const int rpb,
                                                                    const int bufh, const Lens dl)
{
    extern __shared__ float sm[];
    const size_t r0 = row0 + (size_t)blockIdx.x * rpb;
    const int nr = rows - r0 < (size_t)rpb ? (int)(rows - r0) : rpb;
    stage(approx + r0 * n, sm, nr * n, threadIdx.x, WF_BLOCK);
    __syncthreads();
    size_t off = 0;
    for (int l = 0; l < levels; ++l) off += rows * (size_t)dl.v[l];
    float *src = sm, *dst = sm + bufh;
    int c = n;
    for (int s = 0; s < levels; ++s) {
        const int l = levels - 1 - s, ds = dl.v[l];
        off -= rows * (size_t)ds;
        const float *dr0 = det + off + r0 * ds;
        const int len = 2 * c, total = nr * len;
        const bool last_level = s == levels - 1;
        float *og = out + r0 * len;
        const int s0 = last_level ? misalign(og) : 0;
        for (int grp = threadIdx.x; 4 * grp < total + s0; grp += WF_BLOCK) {
            const int lo = 4 * grp - s0;
            const int first = lo < 0 ? -lo : 0, last = total - lo < 4 ? total - lo : 4;
            int r = (lo + first) / len, p = lo + first - r * len;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < first || q >= last) continue;
                const float *ra = src + r * c, *rd = dr0 + (size_t)r * ds;
                v[q] = inv_out<W>([&](int i) { return ra[i]; }, [&](int i) { return rd[i]; }, p, len, c);
                if (!last_level) dst[lo + q] = v[q];
                if (++p == len) {
                    p = 0;
                    ++r;
                }
            }
            if (last_level) store4(og + lo, v, first, last);
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
        c = len;
    }
}

}  // namespace wav
}  // namespace kofft
