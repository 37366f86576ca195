// tables.cpp -- host-side planner recipes of the product (NOT the test oracle).
//
// The device never computes trigonometry: kofft's tables are produced by rounding-
// sensitive recurrences, so they are generated here, with the reference's exact
// order of operations, and uploaded.  Compiled with g++ -ffp-contract=off; fmaf / fma and
// sincosf / sincos come from glibc: Rust's mul_add lowers to the former, and its sin_cos()
// -- `(self.sin(), self.cos())` in std -- is merged by LLVM into the latter on
// x86_64-unknown-linux-gnu.  The pair is requested with ONE explicit sincos call so that the
// tables do not depend on this compiler's own merging heuristics (f64 sincos differs from
// sin / cos in the last bit for ~0.14 % of arguments in glibc 2.35; sincosf never does).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "tables.h"

#include <cmath>

namespace {

template <typename T> struct Num;
template <> struct Num<float> {
    static float pi() { return 3.14159265358979323846f; }  // core::f32::consts::PI
    static void sin_cos(float x, float *s, float *c) { ::sincosf(x, s, c); }
    static float fma(float a, float b, float c) { return fmaf(a, b, c); }
};
template <> struct Num<double> {
    static double pi() { return 3.14159265358979323846; }  // core::f64::consts::PI
    static void sin_cos(double x, double *s, double *c) { ::sincos(x, s, c); }
    static double fma(double a, double b, double c) { return ::fma(a, b, c); }
};

// FftPlanner::get_twiddles (fft.rs:391-405)
template <typename T>
void twiddles(size_t n, T *out)
{
    const size_t half = n / 2;
    const T angle = (-(T)2.0f * Num<T>::pi()) / (T)(float)n;
    T s, c;
    Num<T>::sin_cos(angle, &s, &c);
    T w_re = (T)1, w_im = (T)0;
    for (size_t k = 0; k < half; ++k) {
        out[2 * k] = w_re;
        out[2 * k + 1] = w_im;
        const T prev_re = w_re;
        w_re = Num<T>::fma(w_re, c, -(w_im * s));
        w_im = Num<T>::fma(w_im, c, prev_re * s);
    }
}

// build_twiddle_table (rfft.rs:172-183): cur <- cur.mul(w), un-fused complex product
template <typename T>
void rfft_table(size_t m, T *out)
{
    const T angle = -Num<T>::pi() / (T)(float)m;
    T s, c;
    Num<T>::sin_cos(angle, &s, &c);
    T re = (T)1, im = (T)0;
    for (size_t k = 0; k < m; ++k) {
        out[2 * k] = re;
        out[2 * k + 1] = im;
        const T nre = re * c - im * s;
        const T nim = re * s + im * c;
        re = nre;
        im = nim;
    }
}

// FftPlanner::get_bluestein (fft.rs:411-433): chirp[i] = expi(-a_i), b[i] = expi(a_i) mirrored into the tail of a
// zero-padded length-m buffer, a_i = pi * ((i*i) as f32) / (n as f32).  (b's FFT is taken on the device.)
template <typename T>
void bluestein(size_t n, size_t m, T *chirp, T *b)
{
    for (size_t i = 0; i < 2 * m; ++i) b[i] = (T)0;
    for (size_t i = 0; i < n; ++i) {
        const T angle = Num<T>::pi() * (T)(float)(i * i) / (T)(float)n;
        // Complex::expi (num.rs:123-126): re = cos, im = sin of one sin_cos() call
        Num<T>::sin_cos(-angle, &chirp[2 * i + 1], &chirp[2 * i]);
        Num<T>::sin_cos(angle, &b[2 * i + 1], &b[2 * i]);
    }
    for (size_t i = 1; i < n; ++i) {
        b[2 * (m - i)] = b[2 * i];
        b[2 * (m - i) + 1] = b[2 * i + 1];
    }
}

// ScalarFftImpl::fft_radix4 (fft.rs:1455-1548), the parts that do not depend on the data:
//   perm[i]  = index of the INPUT element that sits at position i after the reference's swap loop (fft.rs:1462-1474;
//              it flips one bit per base-4 digit -- not a digit reversal, which is why the arm is not a DFT from n = 16);
//   w        = for every stage len = 16, 64, .. n, the quarter = len/4 triples (w1, w2, w3)[j] the reference builds by
//              starting at (1, 0) and multiplying (Complex::mul, un-fused) by entries 1, 2, 3 of get_twiddles(len) after
//              every j (fft.rs:1490-1530; the sequence restarts for every block i, so one copy per stage serves all).
//              Triples of consecutive stages follow each other (radix4_triples(n) in all).
template <typename T>
void radix4(size_t n, unsigned *perm, T *w)
{
    for (size_t i = 0; i < n; ++i) perm[i] = (unsigned)i;
    size_t j = 0;
    for (size_t i = 1; i < n; ++i) {
        size_t bit = n >> 2;
        while (j & bit) {
            j ^= bit;
            bit >>= 2;
        }
        j ^= bit;
        if (i < j) {
            const unsigned t = perm[i];
            perm[i] = perm[j];
            perm[j] = t;
        }
    }
    T *tw = new T[n >= 16 ? n : 16];
    size_t off = 0;  // triples written so far
    for (size_t len = 16; len <= n; len <<= 2) {
        twiddles<T>(len, tw);
        const T s_re[3] = {tw[2], tw[4], tw[6]}, s_im[3] = {tw[3], tw[5], tw[7]};
        T re[3] = {(T)1, (T)1, (T)1}, im[3] = {(T)0, (T)0, (T)0};
        const size_t quarter = len / 4;
        for (size_t q = 0; q < quarter; ++q) {
            for (int k = 0; k < 3; ++k) {
                w[2 * (3 * (off + q) + k)] = re[k];
                w[2 * (3 * (off + q) + k) + 1] = im[k];
                const T nre = re[k] * s_re[k] - im[k] * s_im[k];  // Complex::mul (num.rs:161-166), un-fused
                const T nim = re[k] * s_im[k] + im[k] * s_re[k];
                re[k] = nre;
                im[k] = nim;
            }
        }
        off += quarter;
    }
    delete[] tw;
}

}  // namespace

namespace kofft_tables {
size_t radix4_triples(size_t n)
{
    size_t t = 0;
    for (size_t len = 16; len <= n; len <<= 2) t += len / 4;
    return t;
}
void radix4_f32(size_t n, unsigned *perm, float *w) { radix4<float>(n, perm, w); }
void radix4_f64(size_t n, unsigned *perm, double *w) { radix4<double>(n, perm, w); }
void bluestein_f32(size_t n, size_t m, float *chirp, float *b) { bluestein<float>(n, m, chirp, b); }
void bluestein_f64(size_t n, size_t m, double *chirp, double *b) { bluestein<double>(n, m, chirp, b); }
void twiddles_f32(size_t n, float *out) { twiddles<float>(n, out); }
void twiddles_f64(size_t n, double *out) { twiddles<double>(n, out); }
void rfft_table_f32(size_t m, float *out) { rfft_table<float>(m, out); }
void rfft_table_f64(size_t m, double *out) { rfft_table<double>(m, out); }
// window::hann (window.rs:24-28), all arithmetic in f32
void hann_f32(size_t len, float *out)
{
    const float pi = 3.14159265358979323846f;
    for (size_t i = 0; i < len; ++i) out[i] = 0.5f - 0.5f * cosf(2.0f * pi * (float)i / (float)len);
}
// DctPlanner::get_cos_table (dct.rs:50-58) and the sine of dct2_with_table (dct.rs:89-92): the angle
// PI * (k as f32) / (2.0 * (n as f32)), then f32::cos and f32::sin -- two separate libm calls in the reference, so two
// here (glibc's sincosf returns the same bits as the pair; tests/test_dct_tables.py checks against cosf / sinf).
void dct2_table_f32(size_t n, float *cs)
{
    const float pi = 3.14159265358979323846f;
    const float den = 2.0f * (float)n;
    for (size_t k = 0; k < n; ++k) {
        const float a = (pi * (float)k) / den;
        cs[2 * k] = cosf(a);
        cs[2 * k + 1] = sinf(a);
    }
}
// The fast DCT-IV's pre- and post-twiddles: no reference code to follow, so the best f32 value of each entry
void dct4_table_f32(size_t n, float *out)
{
    const double pi = 3.14159265358979323846;
    const size_t m = n / 2;
    for (size_t j = 0; j < m; ++j) {
        const double a = -(pi * (double)(4 * j + 1)) / (double)(4 * n);
        out[2 * j] = (float)cos(a);
        out[2 * j + 1] = (float)sin(a);
    }
    for (size_t k = 0; k < m; ++k) {
        const double b = -(pi * (double)k) / (double)n;
        out[2 * (m + k)] = (float)cos(b);
        out[2 * (m + k) + 1] = (float)sin(b);
    }
}
}  // namespace kofft_tables

// ---- direct DCT / DST tables ---------------------------------------------------------------------------------------------------
#include <algorithm>
#include <thread>
#include <vector>

namespace {
// C[i][k] of one kind: the angle in the reference's order of f32 operations (`i as f32` is exact for n <= 2^24), then ONE libm
// call.  Rust's f32::cos / f32::sin are glibc's cosf / sinf on linux-gnu; each loop of the reference calls only one of them.
void direct_rows(int family, int type, size_t n, size_t ldc, float *c, size_t r0, size_t r1, size_t ib, size_t ie)
{
    const float pi = 3.14159265358979323846f;  // core::f32::consts::PI
    const float nf = (float)n;
    for (size_t i = r0; i < r1; ++i) {
        float *row = c + i * ldc;
        std::fill(row, row + ldc, 0.0f);
        if (i < ib || i >= ie) continue;
        const float fi = (float)i;
        for (size_t k = 0; k < n; ++k) {
            const float fk = (float)k;
            float v;
            if (family == 0) {
                switch (type) {
                case 1: v = cosf((pi / (nf - 1.0f) * fi) * fk); break;            // dct.rs:116, 126
                case 2: v = cosf((pi / nf * (fi + 0.5f)) * fk); break;            // dct.rs:137, 141
                case 3: v = cosf((pi / nf * fi) * (fk + 0.5f)); break;            // dct.rs:152, 156
                default: v = cosf((pi / nf * (fi + 0.5f)) * (fk + 0.5f)); break;  // dct.rs:167, 171
                }
            } else {
                switch (type) {
                case 1: v = sinf(((fi + 1.0f) * (fk + 1.0f)) * (pi / (nf + 1.0f))); break;  // dst.rs:92, 96: the product first
                case 2: v = sinf((pi / nf * (fi + 0.5f)) * (fk + 1.0f)); break;            // dst.rs:107, 111
                case 3: v = sinf((pi / nf * (fk + 0.5f)) * fi); break;                     // dst.rs:122, 126: k first
                default: v = sinf((pi / nf * (fi + 0.5f)) * (fk + 0.5f)); break;           // dst.rs:137, 141
                }
            }
            row[k] = v;
        }
    }
}

template <typename T>
void dst_planner(int type, size_t n, T *out)
{
    const float off = type == 3 ? 0.0f : 0.5f;
    const T factor = Num<T>::pi() / (T)(float)n;
    for (size_t i = 0; i < n; ++i) {
        const T angle = factor * ((T)(float)i + (T)off);
        if constexpr (sizeof(T) == 4) out[i] = sinf(angle);
        else out[i] = ::sin(angle);
    }
}
}  // namespace

namespace kofft_tables {
void direct_range(int family, int type, size_t n, size_t *i_begin, size_t *i_end)
{
    if (family == 0 && type == 1) {  // dct.rs:125: input.iter().take(n - 1).enumerate().skip(1)
        *i_begin = 1;
        *i_end = n >= 2 ? n - 1 : 1;
    } else if (type == 3) {  // dct.rs:155 / dst.rs:125: .skip(1)
        *i_begin = 1;
        *i_end = n >= 1 ? n : 1;
    } else {
        *i_begin = 0;
        *i_end = n;
    }
}
void direct_table_f32(int family, int type, size_t n, size_t ldc, float *c)
{
    size_t ib, ie;
    direct_range(family, type, n, &ib, &ie);
    // at most 16 threads, and none for tables of fewer than 2^16 entries (n = 4096: 16.7 M libm calls)
    size_t threads = std::min<size_t>({size_t(16), std::max<size_t>(1, std::thread::hardware_concurrency()), std::max<size_t>(1, n * n >> 16)});
    if (threads <= 1) {
        direct_rows(family, type, n, ldc, c, 0, n, ib, ie);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; ++t) {
        const size_t r0 = t * per, r1 = std::min(n, r0 + per);
        if (r0 >= r1) break;
        pool.emplace_back(direct_rows, family, type, n, ldc, c, r0, r1, ib, ie);
    }
    for (auto &th : pool) th.join();
}
void dst_planner_f32(int type, size_t n, float *out) { dst_planner<float>(type, n, out); }
void dst_planner_f64(int type, size_t n, double *out) { dst_planner<double>(type, n, out); }
// ---- czt::czt_f32 and goertzel::goertzel_f32 (spectral_impl.hip.h) -----------------------------------------------------------------
// The un-fused complex product the reference spells out three times (czt.rs:28-29, 43-44, 47-48)
static inline void czt_mul(float pr, float pi, float qr, float qi, float *tr, float *ti)
{
    *tr = pr * qr - pi * qi;
    *ti = pr * qi + pi * qr;
}

void czt_wpow_f32(size_t m, float wr, float wi, float *wpow)
{
    float pr = 1.0f, pi = 0.0f;
    for (size_t k = 0; k < m; ++k) {
        wpow[2 * k] = pr;
        wpow[2 * k + 1] = pi;
        czt_mul(pr, pi, wr, wi, &pr, &pi);
    }
}

void czt_apow_f32(size_t n, float ar, float ai, float *apow)
{
    const float denom = ar * ar + ai * ai;
    const float ir = denom == 0.0f ? 0.0f : ar / denom;
    const float ii = denom == 0.0f ? 0.0f : -ai / denom;
    float pr = 1.0f, pi = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        apow[2 * i] = pr;
        apow[2 * i + 1] = pi;
        czt_mul(pr, pi, ir, ii, &pr, &pi);
    }
}

void czt_table_f32(size_t n, size_t m, float wr, float wi, float ar, float ai, size_t ldc, float *c)
{
    if (n == 0 || m == 0) return;
    std::vector<float> wpow(2 * m), apow(2 * n), wnk(2 * m);
    czt_wpow_f32(m, wr, wi, wpow.data());
    czt_apow_f32(n, ar, ai, apow.data());
    for (size_t k = 0; k < m; ++k) {
        wnk[2 * k] = 1.0f;
        wnk[2 * k + 1] = 0.0f;
    }
    for (size_t i = 0; i < n; ++i) {
        float *row = c + i * ldc;
        for (size_t k = 0; k < m; ++k) {
            czt_mul(apow[2 * i], apow[2 * i + 1], wnk[2 * k], wnk[2 * k + 1], &row[2 * k], &row[2 * k + 1]);
            czt_mul(wnk[2 * k], wnk[2 * k + 1], wpow[2 * k], wpow[2 * k + 1], &wnk[2 * k], &wnk[2 * k + 1]);
        }
        for (size_t k = 2 * m; k < ldc; ++k) row[k] = 0.0f;
    }
}

void goertzel_coeff_f32(size_t n, float sample_rate, const float *target_freqs, size_t nfreq, float *coeff)
{
    const float nf = (float)n;
    for (size_t j = 0; j < nfreq; ++j) {
        const float k = floorf((target_freqs[j] * nf) / sample_rate);
        const float omega = ((2.0f * Num<float>::pi()) * k) / nf;
        coeff[j] = 2.0f * cosf(omega);
    }
}

}  // namespace kofft_tables

// ---- hartley::dht and the windows beyond Hann ---------------------------------------------------------------------------------------
#include "libm_trigf.hip.h"

namespace {
void dht_rows(size_t n, size_t ldc, float *h, size_t r0, size_t r1)
{
    const float factor = (2.0f * Num<float>::pi()) / (float)n;  // hartley.rs:15
    for (size_t i = r0; i < r1; ++i) {
        float *row = h + i * ldc;
        for (size_t k = 0; k < n; ++k) {
            const float angle = factor * (float)(i * k);  // hartley.rs:19
            row[k] = kofft::libm_cosf(angle) + kofft::libm_sinf(angle);
        }
        std::fill(row + n, row + ldc, 0.0f);
    }
}

// window.rs:9-21
float bessel0(float x)
{
    float sum = 1.0f;
    const float y = x * x / 4.0f;
    float t = y;
    float k = 1.0f;
    for (int n = 1; n < 20; ++n) {
        k *= (float)n;
        sum += t / (k * k);
        t *= y;
    }
    return sum;
}

// Rust's `as usize` of an f32: NaN and negatives 0, beyond the range usize::MAX
size_t saturating_usize(float v)
{
    if (!(v > 0.0f)) return 0;
    if (v >= 18446744073709551616.0f) return ~size_t(0);
    return (size_t)v;
}
}  // namespace

namespace kofft_tables {
bool libm_trigf(const float *x, size_t count, float *cos_out, float *sin_out)
{
    for (size_t j = 0; j < count; ++j)
        if (!kofft::libm_trigf_in_range(x[j])) return false;
    for (size_t j = 0; j < count; ++j) {
        if (cos_out) cos_out[j] = kofft::libm_cosf(x[j]);
        if (sin_out) sin_out[j] = kofft::libm_sinf(x[j]);
    }
    return true;
}

void dht_table_f32(size_t n, size_t ldc, float *h)
{
    // the thread rule of direct_table_f32
    size_t threads = std::min<size_t>({size_t(16), std::max<size_t>(1, std::thread::hardware_concurrency()), std::max<size_t>(1, n * n >> 16)});
    if (threads <= 1) {
        dht_rows(n, ldc, h, 0, n);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; ++t) {
        const size_t r0 = t * per, r1 = std::min(n, r0 + per);
        if (r0 >= r1) break;
        pool.emplace_back(dht_rows, n, ldc, h, r0, r1);
    }
    for (auto &th : pool) th.join();
}

void window_f32(int kind, size_t len, float param, float *out)
{
    const float pi = Num<float>::pi();  // core::f32::consts::PI
    const float lenf = (float)len;
    switch (kind) {
    case 0:  // hamming, window.rs:31-35: glibc cosf
        for (size_t i = 0; i < len; ++i) out[i] = 0.54f - 0.46f * cosf(2.0f * pi * (float)i / lenf);
        break;
    case 1:  // blackman, window.rs:38-48
        for (size_t i = 0; i < len; ++i) {
            const float x = (float)i / lenf;
            out[i] = 0.42f - 0.5f * cosf(2.0f * pi * x) + 0.08f * cosf(4.0f * pi * x);
        }
        break;
    case 2: {  // kaiser, window.rs:52-61; the crate's sqrtf is the correctly rounded root (NaN below zero)
        const float denom = bessel0(param);
        const float m = (float)(len - 1) / 2.0f;
        for (size_t i = 0; i < len; ++i) {
            const float r = ((float)i - m) / m;
            out[i] = bessel0(param * sqrtf(1.0f - r * r)) / denom;
        }
        break;
    }
    case 3: {  // tukey, window_more.rs:13-28: f32::clamp keeps a NaN, `as usize` saturates, .cos() is glibc's
        float alpha = param;
        if (alpha < 0.0f) alpha = 0.0f;
        if (alpha > 1.0f) alpha = 1.0f;
        const size_t edge = saturating_usize(floorf(alpha * (lenf - 1.0f) / 2.0f));
        for (size_t n = 0; n < len; ++n) {
            if (n < edge) {
                out[n] = 0.5f * (1.0f + cosf(pi * (2.0f * (float)n / (alpha * (lenf - 1.0f)) - 1.0f)));
            } else if (n < len - edge) {
                out[n] = 1.0f;
            } else {
                out[n] = 0.5f * (1.0f + cosf(pi * (2.0f * (float)n / (alpha * (lenf - 1.0f)) - 2.0f / alpha + 1.0f)));
            }
        }
        break;
    }
    case 4:  // bartlett, window_more.rs:31-39
        for (size_t i = 0; i < len; ++i) {
            const float x = ((float)i - (lenf - 1.0f) / 2.0f) / ((lenf - 1.0f) / 2.0f);
            out[i] = 1.0f - fabsf(x);
        }
        break;
    case 5:  // bohman, window_more.rs:42-50: the crate's cosf / sinf
        for (size_t i = 0; i < len; ++i) {
            const float x = ((float)i / (lenf - 1.0f)) - 0.5f;
            out[i] = (1.0f - fabsf(x)) * kofft::libm_cosf(pi * x) + 1.0f / pi * kofft::libm_sinf(pi * x);
        }
        break;
    default:  // nuttall, window_more.rs:53-64: the crate's cosf
        for (size_t n = 0; n < len; ++n) {
            const float x = 2.0f * pi * (float)n / (lenf - 1.0f);
            out[n] = 0.355768f - 0.487396f * kofft::libm_cosf(x) + 0.144232f * kofft::libm_cosf(2.0f * x) -
                     0.012604f * kofft::libm_cosf(3.0f * x);
        }
        break;
    }
}

// ---- cepstrum::mel_filterbank: the edges and the kernels' plan ----------------------------------------------------------------------
void mel_bins_f32(float sample_rate, size_t n_fft, size_t num_filters, uint64_t *bins)
{
    const float f_min = 0.0f;
    const float f_max = sample_rate / 2.0f;                          // cepstrum.rs:39
    const float mel_min = 2595.0f * log10f(1.0f + f_min / 700.0f);   // cepstrum.rs:40
    const float mel_max = 2595.0f * log10f(1.0f + f_max / 700.0f);   // cepstrum.rs:41
    for (size_t i = 0; i < num_filters + 2; ++i) {
        float p = mel_min + (mel_max - mel_min) * (float)i / (float)(num_filters + 1);  // cepstrum.rs:44: ((d * i) / (M + 1))
        p = 700.0f * (powf(10.0f, p / 2595.0f) - 1.0f);                                 // cepstrum.rs:45
        bins[i] = saturating_usize(floorf(p * ((float)n_fft + 1.0f) / sample_rate));    // cepstrum.rs:49
    }
}

size_t mel_plan_ints(size_t num_mel) { return 2 * (num_mel + 1) + num_mel; }

void mel_plan_build(const uint64_t *bins, size_t n_fft, size_t num_mel, int *ints, float *w)
{
    int *seg = ints, *live = ints + 2 * (num_mel + 1);
    for (size_t k = 0; k < 2 * n_fft; ++k) w[k] = 0.0f;
    for (size_t s = 0; s <= num_mel; ++s) {
        const uint64_t a = bins[s], b = bins[s + 1];
        const uint64_t lo = a < n_fft ? a : n_fft, hi = b < n_fft ? b : n_fft;
        seg[2 * s] = (int)lo;
        seg[2 * s + 1] = (int)hi;
        const float d = (float)(b - a);  // cepstrum.rs:59, 64: `(bins[m] - bins[m - 1]) as f32`
        for (uint64_t k = lo; k < hi; ++k) {
            w[2 * k] = (float)(k - a) / d;
            w[2 * k + 1] = (float)(b - k) / d;
        }
    }
    for (size_t m = 0; m < num_mel; ++m) live[m] = (bins[m + 1] != bins[m] && bins[m + 2] != bins[m + 1]) ? 1 : 0;
}

// ---- visual::spectrogram: the log-frequency map and the kernels' pixel ranges -----------------------------------------------------
void log_bin_map(size_t bins, uint32_t *pix_of_bin)
{
    if (bins == 0) return;
    const size_t max_bin = bins - 1;
    const float log_max = logf((float)max_bin + 1.0f);  // spectrogram.rs:213
    for (size_t b = 0; b < bins; ++b) {
        if (max_bin == 0) {
            pix_of_bin[b] = 0;  // spectrogram.rs:210
            continue;
        }
        const float pos = logf((float)b + 1.0f);                                              // spectrogram.rs:214
        const uint64_t y = saturating_usize(floorf((float)max_bin * pos / log_max));          // spectrogram.rs:215
        pix_of_bin[b] = y > 0xffffffffull ? 0xffffffffu : (uint32_t)y;
    }
}

bool spec_ranges_build(const uint32_t *pix_of_bin, size_t bins, uint32_t *start)
{
    size_t p = 0;  // the next pixel whose first bin is not known yet
    for (size_t b = 0; b < bins; ++b) {
        const uint32_t y = pix_of_bin[b];
        if (y >= bins || (b > 0 && y < pix_of_bin[b - 1])) return false;
        for (; p <= y; ++p) start[p] = (uint32_t)b;
    }
    for (; p <= bins; ++p) start[p] = (uint32_t)bins;
    return true;
}

}  // namespace kofft_tables
