// tables.h -- host-side planner recipes (see tables.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
namespace kofft_tables {
void twiddles_f32(size_t n, float *out);   // n/2 complex
void twiddles_f64(size_t n, double *out);
void rfft_table_f32(size_t m, float *out); // m complex
void rfft_table_f64(size_t m, double *out);
void hann_f32(size_t len, float *out);
// DctPlanner (dct.rs:50-58, 89-92): n (cos, sin) pairs of a_k = (PI * k) / (2 * n), all in f32
void dct2_table_f32(size_t n, float *cs);
// The fast DCT-IV's two twiddle tables, n even and M = n / 2: M (cos, sin) pairs of a_j = -PI (4j + 1) / (4n), then
// M pairs of b_k = -PI k / n; every angle and every cos / sin in double, rounded once to f32
void dct4_table_f32(size_t n, float *out);
// dct::dct1..dct4 (dct.rs:108-176) and dst::dst1..dst4 (dst.rs:89-146): the n x n table C[i][k] (row-major, row stride ldc >= n)
// of the direct sums, each entry glibc cosf / sinf of the reference's angle; rows outside the kind's i range are zero, so are
// columns n .. ldc-1.  family 0 = DCT, 1 = DST; type 1..4.  Built on up to 16 host threads.
void direct_range(int family, int type, size_t n, size_t *i_begin, size_t *i_end);
void direct_table_f32(int family, int type, size_t n, size_t ldc, float *c);
// DstPlanner::build_table_offset (dst.rs:41-50): sin(factor * (i + off)), factor = pi_T / T::from_f32(n as f32); off 0.5 (type 2,
// 4) or 0.0 (type 3)
void dst_planner_f32(int type, size_t n, float *out);
void dst_planner_f64(int type, size_t n, double *out);
void bluestein_f32(size_t n, size_t m, float *chirp /* n complex */, float *b /* m complex */);
void bluestein_f64(size_t n, size_t m, double *chirp, double *b);
// fft_radix4 (fft.rs:1455-1548), n a power of four: perm = n source indices, w = radix4_triples(n) x (w1, w2, w3) complex
size_t radix4_triples(size_t n);
void radix4_f32(size_t n, unsigned *perm, float *w);
void radix4_f64(size_t n, unsigned *perm, double *w);
// czt::czt_f32 (czt.rs:16-54), all f32 and unfused.  wpow: m complex, wpow[k] = w multiplied k times into (1, 0) (czt.rs:25-32; the
// reference restarts at every k, a running prefix gives the same bits).  apow: n complex, apow[i] = a_inv multiplied i times into
// (1, 0), a_inv = (ar / denom, -ai / denom), denom = ar * ar + ai * ai, (0, 0) at denom == 0 (czt.rs:19-21, 47-50).
void czt_wpow_f32(size_t m, float wr, float wi, float *wpow);
void czt_apow_f32(size_t n, float ar, float ai, float *apow);
// The table of the chirp-Z sums: C[i][2k], C[i][2k + 1] = apow[i] * wpow[k]^i (czt.rs:38-46), n rows of 2 m floats, row stride
// ldc >= 2 m; columns 2 m .. ldc - 1 are +0.  The host restatement of what czt_recur_kernel<TABLE> builds on the device.
void czt_table_f32(size_t n, size_t m, float wr, float wi, float ar, float ai, size_t ldc, float *c);
// goertzel::goertzel_f32 (goertzel.rs:23-26): coeff[j] = 2 * cosf(((2 * PI) * floorf((f_j * n) / rate)) / n), n as f32, glibc cosf
void goertzel_coeff_f32(size_t n, float sample_rate, const float *target_freqs, size_t nfreq, float *coeff);
// The libm crate's cosf / sinf (libm_trigf.hip.h compiled for the host) of count arguments; either output may be null.  False, and
// nothing written, if an argument needs rem_pio2_large (a finite |x| >= 0x4dc90fdb), which the header does not restate.
bool libm_trigf(const float *x, size_t count, float *cos_out, float *sin_out);
// hartley::dht (hartley.rs:12-27): H[i][k] = cosf(a) + sinf(a), a = factor * ((i * k) as f32), factor = (2.0 * PI) / n as f32, the
// crate's cosf / sinf and one f32 add; n rows of ldc >= n floats, columns n .. ldc - 1 are +0.  Built on up to 16 host threads; the
// host restatement of what dht_table_kernel (hartley_impl.hip.h) builds on the device.
void dht_table_f32(size_t n, size_t ldc, float *h);
// window::hamming / blackman / kaiser (window.rs:31-61) and window_more::tukey / bartlett / bohman / nuttall (window_more.rs:13-64),
// kind = KOFFT_WINDOW_* of include/kofft_hip.h (0 .. 6), all arithmetic in f32 in Rust's parse order; param: kaiser's beta, tukey's
// alpha, ignored otherwise.  The caller has checked the kind and, for kaiser, len != 0.
void window_f32(int kind, size_t len, float param, float *out);
constexpr int kWindowKinds = 7;
// cepstrum::mel_filterbank's edges (cepstrum.rs:38-50) in f32 in Rust's parse order, with glibc's log10f / powf where the reference
// calls the libm crate's, and the saturating `floorf(..) as usize`: bins = num_filters + 2 values.
void mel_bins_f32(float sample_rate, size_t n_fft, size_t num_filters, uint64_t *bins);
// What the filterbank kernels walk (mfcc_impl.hip.h), from nondecreasing edges bins[0 .. num_mel + 1] and rows of n_fft <= 2^24 values.
// Segment s = [bins[s], bins[s + 1]) is the rise of filter s and the fall of filter s - 1 (cepstrum.rs:57-66):
//   seg[2 s], seg[2 s + 1]  its bounds clamped to n_fft (the reference skips k >= n_fft; the unclamped edges still set the denominators)
//   live[m]                 1 unless bins[m + 1] == bins[m] or bins[m + 2] == bins[m + 1] (cepstrum.rs:54: the filter stays +0)
//   w[2 k], w[2 k + 1]      for k < n_fft inside a segment s: ((k - bins[s]) as f32) / d and ((bins[s + 1] - k) as f32) / d,
//                           d = (bins[s + 1] - bins[s]) as f32, conversions rounded to nearest, the division correctly rounded;
//                           +0 for every k outside [bins[0], bins[num_mel + 1])
// ints: 2 (num_mel + 1) + num_mel values (seg, then live); w: 2 n_fft floats.
size_t mel_plan_ints(size_t num_mel);
void mel_plan_build(const uint64_t *bins, size_t n_fft, size_t num_mel, int *ints, float *w);
// visual::spectrogram::map_bin_to_pixel(b, bins - 1) for every b < bins (spectrogram.rs:209-217): f32 in Rust's parse order with glibc's
// logf, max_bin == 0 -> 0, the saturating `floor(..) as usize` clamped to 32 bits.
void log_bin_map(size_t bins, uint32_t *pix_of_bin);
// The pixel ranges the render kernels walk (spectrogram_impl.hip.h) from a bin -> pixel table: pixel p averages the bins
// [start[p], start[p + 1]), p < bins; start holds bins + 1 values, start[bins] == bins.  false, with start undefined: an entry >= bins,
// or a table that is not nondecreasing (its pixels would not be ranges).
bool spec_ranges_build(const uint32_t *pix_of_bin, size_t bins, uint32_t *start);
}  // namespace kofft_tables
