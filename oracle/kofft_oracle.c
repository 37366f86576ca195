/*
 * kofft_oracle.c -- CPU oracle for the kofft hot path.  TEST INFRASTRUCTURE ONLY;
 * see kofft_oracle.h for who may load it and for the pinning status.
 *
 * Build: gcc -O2 -ffp-contract=off -fPIC -shared (oracle/Makefile).  No -march flags:
 * the reference's default build has no FMA, so products and sums round separately.
 */
#include "kofft_oracle.h"

#ifndef _GNU_SOURCE
#define _GNU_SOURCE /* sincosf / sincos */
#endif
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ---- f32 instantiation ---- */
#define REAL float
#define SFX(name) name##_f32
#define RSINCOS sincosf
#define RCOS cosf
#define RFMA fmaf
/* core::f32::consts::PI (num.rs:2, 57-59) */
#define R_PI 3.14159265358979323846f
#include "kofft_oracle_impl.inc"
#undef REAL
#undef SFX
#undef RSINCOS
#undef RCOS
#undef RFMA
#undef R_PI

/* ---- f64 instantiation ---- */
#define REAL double
#define SFX(name) name##_f64
#define RSINCOS sincos
#define RCOS cos
#define RFMA fma
/* core::f64::consts::PI (num.rs:91-93) */
#define R_PI 3.14159265358979323846
#include "kofft_oracle_impl.inc"
#undef REAL
#undef SFX
#undef RSINCOS
#undef RCOS
#undef RFMA
#undef R_PI

/* window.rs:24-28  hann(len): 0.5 - 0.5 * cos(2.0 * PI * i as f32 / len as f32), all f32 */
int ko_hann_f32(size_t len, float *out)
{
    const float pi = 3.14159265358979323846f;
    for (size_t i = 0; i < len; ++i)
        out[i] = 0.5f - 0.5f * cosf(2.0f * pi * (float)i / (float)len);
    return KO_OK;
}

/* stft.rs:91-103  one frame: window-multiply / zero-pad, then the full complex FFT */
static int stft_frame(ko_planner_f32 *p, const float *signal, size_t len, const float *window,
                      size_t win_len, size_t start, float *frame)
{
    for (size_t i = 0; i < win_len; ++i) {
        float x = (start + i < len) ? signal[start + i] * window[i] : 0.0f;
        frame[2 * i] = x;
        frame[2 * i + 1] = 0.0f;
    }
    return ko_fft_p_f32(p, frame, win_len);
}

/* stft.rs:76-105  stft(): hop==0 -> InvalidHopSize; fewer than ceil(len/hop) frames ->
 * MismatchedLengths; EVERY provided frame is computed (not only the required ones).
 * A zero-length window reaches fft.fft(&mut []) -> EmptyInput (fft.rs:1056). */
int ko_stft_f32(const float *signal, size_t len, const float *window, size_t win_len, size_t hop,
                float *out, size_t frames)
{
    if (hop == 0) return KO_ERR_INVALID_HOP_SIZE;
    size_t required = (len + hop - 1) / hop;
    if (frames < required) return KO_ERR_MISMATCHED_LENGTHS;
    return ko_stft_range_f32(signal, len, window, win_len, hop, out, 0, frames);
}

int ko_stft_range_f32(const float *signal, size_t len, const float *window, size_t win_len,
                      size_t hop, float *out, size_t first, size_t count)
{
    if (hop == 0) return KO_ERR_INVALID_HOP_SIZE;
    ko_planner_f32 *p = ko_planner_new_f32();
    if (!p) return KO_ERR_ALLOC;
    int rc = KO_OK;
    for (size_t f = 0; f < count && rc == KO_OK; ++f)
        rc = stft_frame(p, signal, len, window, win_len, (first + f) * hop, out + 2 * win_len * f);
    ko_planner_free_f32(p);
    return rc;
}

/* stft.rs:117-156  istft(): overlap-add with window^2 normalisation (> 1e-8 guard).
 * frames_data (frames*win_len complex) is transformed in place, like the reference's
 * &mut frames.  `output` is accumulated into (+=): the reference does not clear it. */
int ko_istft_f32(float *frames_data, size_t frames, const float *window, size_t win_len,
                 size_t hop, float *output, size_t out_len, float *scratch, size_t scratch_len)
{
    if (hop == 0) return KO_ERR_INVALID_HOP_SIZE;
    if (scratch_len != out_len) return KO_ERR_MISMATCHED_LENGTHS;
    for (size_t i = 0; i < scratch_len; ++i) scratch[i] = 0.0f;
    ko_planner_f32 *p = ko_planner_new_f32();
    if (!p) return KO_ERR_ALLOC;
    int rc = KO_OK;
    for (size_t f = 0; f < frames && rc == KO_OK; ++f) {
        size_t start = f * hop;
        float *frame = frames_data + 2 * win_len * f;
        rc = ko_ifft_p_f32(p, frame, win_len);
        if (rc) break;
        for (size_t i = 0; i < win_len; ++i) {
            if (start + i < out_len) {
                output[start + i] += frame[2 * i] * window[i];
                scratch[start + i] += window[i] * window[i];
            }
        }
    }
    ko_planner_free_f32(p);
    if (rc) return rc;
    for (size_t i = 0; i < out_len; ++i)
        if (scratch[i] > 1e-8f) output[i] /= scratch[i];
    return KO_OK;
}

/* visual::spectrogram::stft_magnitudes (visual/spectrogram.rs:52-76): window = hann(win_len) (window.rs:24-28), frames =
 * ceil(len / hop) STFT frames (compute_stft = stft.rs:76-105), then for the first win_len/2 bins of every frame
 *   mag = (c.re * c.re + c.im * c.im).sqrt()        -- f32, un-fused, correctly rounded sqrt (spectrogram.rs:66)
 *   if mag > max_mag { max_mag = mag }              -- a NaN is never selected (spectrogram.rs:68-70)
 * mags: frames * (win_len/2) floats, row-major.  hop == 0: the reference divides by it (div_ceil) and panics. */
int ko_stft_magnitudes_f32(const float *samples, size_t len, size_t win_len, size_t hop, float *mags, float *max_mag)
{
    if (hop == 0) return KO_ERR_INVALID_HOP_SIZE;
    const size_t frames = (len + hop - 1) / hop;
    const size_t height = win_len / 2;
    *max_mag = 0.0f;
    if (frames == 0) return KO_OK;
    float *window = (float *)malloc((win_len ? win_len : 1) * sizeof(float));
    float *spec = (float *)malloc((frames * win_len * 2 + 1) * sizeof(float));
    if (!window || !spec) {
        free(window);
        free(spec);
        return KO_ERR_ALLOC;
    }
    ko_hann_f32(win_len, window);
    int rc = ko_stft_f32(samples, len, window, win_len, hop, spec, frames);
    if (rc == KO_OK) {
        float mx = 0.0f;
        for (size_t x = 0; x < frames; ++x) {
            for (size_t y = 0; y < height; ++y) {
                const float re = spec[2 * (x * win_len + y)], im = spec[2 * (x * win_len + y) + 1];
                const float rr = re * re, ii = im * im;
                const float mag = sqrtf(rr + ii);
                mags[x * height + y] = mag;
                if (mag > mx) mx = mag;
            }
        }
        *max_mag = mx;
    }
    free(window);
    free(spec);
    return rc;
}

/* ---- direct DCT-I..IV (dct.rs:108-176) / DST-I..IV (dst.rs:89-146), f32 ------------------------------------------------------
 * The reference's loops: for every k, sum = seed; for i in its range, sum += x[i] * f(angle(i, k)), f = cos (DCT) / sin (DST),
 * angle in f32 in the reference's order of operations, f32::cos / f32::sin = glibc cosf / sinf on linux-gnu.  Here the angle
 * table is made once per (family, type, n) and the sum runs over increasing i for a block of outputs k at a time (vectorised over
 * k only; with -ffp-contract=off every term is one rounded multiply and one rounded add, like the reference's). */
static int direct_kind_ok(int family, int type) { return (family == 0 || family == 1) && type >= 1 && type <= 4; }

/* the i of the inner loop: dct1 take(n - 1).skip(1); dct3 / dst3 skip(1); the rest every i */
static void direct_i_range(int family, int type, size_t n, size_t *lo, size_t *hi)
{
    *lo = 0;
    *hi = n;
    if (family == 0 && type == 1) {
        *lo = 1;
        *hi = n > 1 ? n - 1 : 1;
    } else if (type == 3) {
        *lo = 1;
    }
}

static float direct_angle(int family, int type, float nf, float fi, float fk)
{
    const float pi = 3.14159265358979323846f; /* core::f32::consts::PI */
    if (family == 0) {
        if (type == 1) return ((pi / (nf - 1.0f)) * fi) * fk;       /* factor * i as f32 * k as f32 */
        const float f = pi / nf;
        if (type == 2) return (f * (fi + 0.5f)) * fk;
        if (type == 3) return (f * fi) * (fk + 0.5f);
        return (f * (fi + 0.5f)) * (fk + 0.5f);
    }
    if (type == 1) return ((fi + 1.0f) * (fk + 1.0f)) * (pi / (nf + 1.0f)); /* (i + 1) * (k + 1) * factor */
    const float f = pi / nf;
    if (type == 2) return (f * (fi + 0.5f)) * (fk + 1.0f);
    if (type == 3) return (f * (fk + 0.5f)) * fi;
    return (f * (fi + 0.5f)) * (fk + 0.5f);
}

int ko_direct_table_rows_f32(int family, int type, size_t n, size_t first, size_t count, float *out)
{
    if (!direct_kind_ok(family, type)) return KO_ERR_INVALID_VALUE;
    size_t lo, hi;
    direct_i_range(family, type, n, &lo, &hi);
    const float nf = (float)n;
    for (size_t r = 0; r < count; ++r) {
        const size_t i = first + r;
        float *row = out + r * n;
        if (i < lo || i >= hi) {
            for (size_t k = 0; k < n; ++k) row[k] = 0.0f;
            continue;
        }
        for (size_t k = 0; k < n; ++k) {
            const float a = direct_angle(family, type, nf, (float)i, (float)k);
            row[k] = family == 0 ? cosf(a) : sinf(a);
        }
    }
    return KO_OK;
}

int ko_direct_table_f32(int family, int type, size_t n, float *out)
{
    return ko_direct_table_rows_f32(family, type, n, 0, n, out);
}

#define DIRECT_ROWS 16  /* rows of x per block: each table row is read once per block */
#define DIRECT_COLS 512 /* outputs per block: DIRECT_ROWS x DIRECT_COLS running sums stay in L1 / L2 */

int ko_direct_tab_f32(const float *table, int family, int type, const float *x, float *out, size_t n, size_t batch)
{
    if (!direct_kind_ok(family, type)) return KO_ERR_INVALID_VALUE;
    if (n == 0) return KO_OK;
    size_t lo, hi;
    direct_i_range(family, type, n, &lo, &hi);
    const int dct1 = family == 0 && type == 1;
    for (size_t b0 = 0; b0 < batch; b0 += DIRECT_ROWS) {
        const size_t nb = batch - b0 < DIRECT_ROWS ? batch - b0 : DIRECT_ROWS;
        for (size_t k0 = 0; k0 < n; k0 += DIRECT_COLS) {
            const size_t nk = n - k0 < DIRECT_COLS ? n - k0 : DIRECT_COLS;
            /* the seed: dct1 input[0] + (+-input[n - 1]) (n == 1: input[0] * 2.0), dct3 / dst3 input[0] / 2.0, else +0 */
            for (size_t b = 0; b < nb; ++b) {
                const float *xr = x + (b0 + b) * n;
                float *acc = out + (b0 + b) * n + k0;
                for (size_t k = 0; k < nk; ++k) {
                    float s = 0.0f;
                    if (dct1)
                        s = n == 1 ? xr[0] * 2.0f : (((k0 + k) % 2 == 0) ? xr[0] + xr[n - 1] : xr[0] + (-xr[n - 1]));
                    else if (type == 3)
                        s = xr[0] / 2.0f;
                    acc[k] = s;
                }
            }
            for (size_t i = lo; i < hi; ++i) {
                const float *c = table + i * n + k0;
                for (size_t b = 0; b < nb; ++b) {
                    const float xi = dct1 ? 2.0f * x[(b0 + b) * n + i] : x[(b0 + b) * n + i];
                    float *acc = out + (b0 + b) * n + k0;
                    for (size_t k = 0; k < nk; ++k) acc[k] = acc[k] + xi * c[k];
                }
            }
        }
    }
    return KO_OK;
}

int ko_direct_f32(int family, int type, const float *x, float *out, size_t n, size_t batch)
{
    if (!direct_kind_ok(family, type)) return KO_ERR_INVALID_VALUE;
    if (n == 0) return KO_OK;
    float *table = (float *)malloc(n * n * sizeof(float));
    if (!table) return KO_ERR_ALLOC;
    int rc = ko_direct_table_f32(family, type, n, table);
    if (rc == KO_OK) rc = ko_direct_tab_f32(table, family, type, x, out, n, batch);
    free(table);
    return rc;
}

const char *ko_strerror(int code)
{
    switch (code) {
    case KO_OK: return "Ok";
    case KO_ERR_EMPTY_INPUT: return "FftError::EmptyInput";
    case KO_ERR_NON_POWER_OF_TWO_NO_STD: return "FftError::NonPowerOfTwoNoStd";
    case KO_ERR_MISMATCHED_LENGTHS: return "FftError::MismatchedLengths";
    case KO_ERR_INVALID_STRIDE: return "FftError::InvalidStride";
    case KO_ERR_INVALID_HOP_SIZE: return "FftError::InvalidHopSize";
    case KO_ERR_INVALID_VALUE: return "FftError::InvalidValue";
    case KO_ERR_UNSUPPORTED: return "oracle: non-power-of-two length (Bluestein arm not restated)";
    case KO_ERR_ALLOC: return "oracle: allocation failure";
    default: return "unknown";
    }
}
