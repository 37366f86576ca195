/*
 * kofft_hip.h -- C ABI of the MI355X (gfx950) implementation of kofft's hot path:
 * batched power-of-two complex FFT, real-FFT post-pass, windowed STFT.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface
 * (okian/kofft v0.1.5, file:line) it stands in for; a Rust shim implementing
 * kofft's `FftImpl<T>` trait (fft.rs:466-587) binds exactly these symbols --
 * see INTEGRATION.md for the shim and for the C++/Python host mirrors.
 *
 * Conventions
 *   - Complex data is interleaved {re, im}: kofft's #[repr(C)] Complex<T>
 *     (num.rs:105-110; tests/complex_repr.rs proves [T;2] compatibility), so a
 *     `&mut [Complex32]` passes as `float*` with 2*len floats.
 *   - Plain pointers and sizes only.  No torch / HIP types in any signature; a
 *     HIP stream crosses as `void*`.
 *   - Return value: 0 = Ok; 1..6 = kofft's FftError variants in declaration order
 *     (fft.rs:447-454); negative = runtime failure that FftError cannot express
 *     (the shim maps those to a panic).
 *   - `*_dev` entry points take DEVICE pointers, enqueue on the context's stream and
 *     return without synchronising.  The un-suffixed twins take HOST pointers, stage
 *     through device memory and return after the result is back in the host buffer.
 *   - A context is cheap, owns its twiddle-table cache (the role of FftPlanner,
 *     fft.rs:332-408) and is NOT thread-safe: one context per thread, exactly like
 *     ScalarFftImpl (Send + !Sync, fft.rs:589-605).
 *   - Arithmetic: every butterfly performs the reference's un-fused operations with
 *     the reference's recurrence-generated twiddle tables (generated on the host with
 *     the reference's recipe and uploaded; no device-side trigonometry).
 *   - Lengths: complex transforms take any n up to 2^26 (powers of two) / 2^25 (others:
 *     the reference's Bluestein arm, fft.rs:1088-1132, built from the same kernels).
 *     rfft / irfft (half length), stft / istft / stft_magnitudes (window length) and every
 *     axis of the 2-D / 3-D transforms take the same range: powers of two up to 2^14 (f32) /
 *     2^13 (f64) run fused in one kernel, anything else is composed from the complex
 *     transform plus pack / post-pass kernels (the reference calls fft.fft on any length too:
 *     rfft.rs:447, stft.rs:102).  Beyond that range: KOFFT_ERR_UNSUPPORTED, never a wrong answer.
 */
#ifndef KOFFT_HIP_H
#define KOFFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------- */
#define KOFFT_OK 0
/* FftError (fft.rs:447-454), discriminant + 1 */
#define KOFFT_ERR_EMPTY_INPUT 1
#define KOFFT_ERR_NON_POWER_OF_TWO_NO_STD 2
#define KOFFT_ERR_MISMATCHED_LENGTHS 3
#define KOFFT_ERR_INVALID_STRIDE 4
#define KOFFT_ERR_INVALID_HOP_SIZE 5
#define KOFFT_ERR_INVALID_VALUE 6
/* outside FftError */
#define KOFFT_ERR_HIP (-1)         /* a HIP runtime call failed; see kofft_hip_last_error */
#define KOFFT_ERR_UNSUPPORTED (-2) /* length not supported by the device path */
#define KOFFT_ERR_NULL (-3)        /* null context / pointer */
#define KOFFT_ERR_ALLOC (-4)       /* host or device allocation failed */
#define KOFFT_ERR_RCCL (-5)        /* RCCL unavailable or a collective failed; see kofft_hip_multi_last_error */

typedef struct kofft_hip_ctx kofft_hip_ctx;

/* Human-readable name of a status code (static string). */
const char *kofft_hip_strerror(int status);
/* Text of the last HIP failure seen by this context ("" if none). */
const char *kofft_hip_last_error(const kofft_hip_ctx *ctx);
/* Library version string, e.g. "kofft-hip 0.1.0 (gfx950)". */
const char *kofft_hip_version(void);

/* ---- context: stands in for ScalarFftImpl::<T>::default() + its FftPlanner ----
 * (fft.rs:600-613, 332-366).  `device` is the HIP device ordinal. */
int kofft_hip_device_count(int *count);
int kofft_hip_create(int device, kofft_hip_ctx **out);
int kofft_hip_destroy(kofft_hip_ctx *ctx);
/* Use a caller-owned hipStream_t (passed as void*) for all *_dev work; NULL restores
 * the context's own stream. */
int kofft_hip_set_stream(kofft_hip_ctx *ctx, void *hip_stream);
int kofft_hip_synchronize(kofft_hip_ctx *ctx);
/* The context's scratch (host-pointer staging, the large-n intermediate, the Bluestein and composed-length work buffers)
 * only grows with the largest call seen; this synchronises the stream and frees it all (tables stay cached). */
int kofft_hip_release_scratch(kofft_hip_ctx *ctx);
/* (no counterpart in kofft) The large-n path (n beyond one workgroup: two or three factor kernels through an intermediate the
 * context owns) chooses the PLACEMENT of that intermediate: the first call that needs it (full chunks of >= 128 MiB) allocates
 * KOFFT_HIP_BIG_PROBE (default 5, at most 8; 0 / 1 = off) candidates, times its own factor kernels on one chunk of scratch data
 * through each and keeps the fastest (the same kernel reads a 512 MiB hipMalloc at 188 or at 225 us depending on
 * where it lies, for the allocation's lifetime).  This reports the last probe: n candidates, per candidate the first factor's
 * and the whole chunk's time in microseconds (arrays of `cap` floats, may be NULL), and which one was kept (n = 0: no probe ran). */
int kofft_hip_big_probe_info(kofft_hip_ctx *ctx, float *first_us, float *total_us, int cap, int *n, int *pick);

/* ---- tables: the planner recipes, on the host --------------------------------
 * kofft_hip_twiddles_*: FftPlanner::get_twiddles(n) (fft.rs:370-408), n/2 complex.
 * kofft_hip_rfft_table_*: build_twiddle_table(m) (rfft.rs:172-183), m complex.
 * kofft_hip_hann_f32: window::hann(len) (window.rs:24-28).
 * kofft_hip_dct2_table_f32: DctPlanner's (cos, sin) of PI * k / (2n), k < n (dct.rs:50-58, 89-92), n pairs. */
int kofft_hip_twiddles_f32(size_t n, float *out);
int kofft_hip_twiddles_f64(size_t n, double *out);
int kofft_hip_rfft_table_f32(size_t m, float *out);
int kofft_hip_rfft_table_f64(size_t m, double *out);
int kofft_hip_hann_f32(size_t len, float *out);
int kofft_hip_dct2_table_f32(size_t n, float *cs);

/* ---- complex FFT --------------------------------------------------------------
 * FftImpl::fft / FftImpl::ifft (fft.rs:467-468; ScalarFftImpl fft.rs:1054-1082,
 * 1134-1174) applied in place to `batch` contiguous transforms of length n:
 * fft::batch / batch_inverse (fft.rs:2156-2175) over a contiguous layout.
 * data: batch*n complex.  inverse != 0 selects ifft (conj, fft, conj, *1/n).
 * batch == 0 -> KOFFT_OK (batch() over an empty slice); otherwise n == 0 ->
 * KOFFT_ERR_EMPTY_INPUT; n == 1 is a no-op for both directions. */
int kofft_hip_fft_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch, int inverse);
int kofft_hip_fft_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch, int inverse);
int kofft_hip_fft_c32_dev(kofft_hip_ctx *ctx, float *d_data, size_t n, size_t batch, int inverse);
int kofft_hip_fft_c64_dev(kofft_hip_ctx *ctx, double *d_data, size_t n, size_t batch, int inverse);
/* FftImpl::fft_out_of_place / ifft_out_of_place (fft.rs:469-490), device pointers.
 * d_in and d_out must not partially overlap (d_in == d_out is allowed). */
int kofft_hip_fft_c32_dev_oop(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n,
                              size_t batch, int inverse);
int kofft_hip_fft_c64_dev_oop(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n,
                              size_t batch, int inverse);

/* ---- planar (split re / im) complex FFT ------------------------------------------
 * FftImpl::fft_split / ifft_split (fft.rs:1365-1439; FftPlan::fft_split, fft_split_complex,
 * fft_complex_vec: fft.rs:2081-2153) on `batch` contiguous transforms of length n whose real
 * and imaginary parts lie in two separate planes of batch * n reals each -- the reference's
 * SoA layout (SplitComplex, ComplexVec: num.rs:236-308).  The result re + i im is
 * kofft_hip_fft_c32 / _c64 of the interleaved data bit for bit, both directions (inverse != 0:
 * im = -im, the transform, im = -im, re *= 1/n, im *= 1/n); n == 1 leaves both planes as they
 * are.  Checks, in the order of kofft_hip_fft_c32 and before the context is touched:
 * batch == 0 -> KOFFT_OK; n == 0 -> EMPTY_INPUT; n beyond the complex transform's range
 * (2^26 for powers of two, 2^25 otherwise) -> KOFFT_ERR_UNSUPPORTED; a null pointer or
 * context -> KOFFT_ERR_NULL.  Host form: in place.  kofft_hip_dev_*: device pointers (named
 * like kofft_hip_dev_czt_f32), asynchronous on the context's stream; d_re_in == d_re_out and d_im_in == d_im_out (in place) are allowed,
 * any other overlap between the four planes is undefined.  Planes need only the alignment of
 * their element (4 / 8 bytes).  Powers of two 2 .. 2^14 (f32) / 2 .. 2^13 (f64) run in one
 * launch on the planes themselves; every other length -- and, after
 * kofft_hip_set_split_fused(ctx, 0), every length of that context -- is packed into
 * interleaved rows, transformed and unpacked (the same bytes; A/B measurements and tests).
 * (One corner: the f64 ifft_split scales by 1 / (n as f64) where ifft scales by
 * 1 / (n as f32 as f64); the two differ only for lengths above 2^24 that f32 cannot hold,
 * and this entry follows ifft there.) */
int kofft_hip_fft_split_c32(kofft_hip_ctx *ctx, float *re, float *im, size_t n, size_t batch, int inverse);
int kofft_hip_fft_split_c64(kofft_hip_ctx *ctx, double *re, double *im, size_t n, size_t batch, int inverse);
int kofft_hip_dev_fft_split_c32(kofft_hip_ctx *ctx, const float *d_re_in, const float *d_im_in, float *d_re_out, float *d_im_out,
                                size_t n, size_t batch, int inverse);
int kofft_hip_dev_fft_split_c64(kofft_hip_ctx *ctx, const double *d_re_in, const double *d_im_in, double *d_re_out, double *d_im_out,
                                size_t n, size_t batch, int inverse);
int kofft_hip_set_split_fused(kofft_hip_ctx *ctx, int on);

/* ScalarFftImpl::fft_radix4 (fft.rs:1455-1548) byte for byte.  kofft's fft_with_strategy(.., FftStrategy::Radix4)
 * (fft.rs:1356) runs it for powers of four, and from n = 16 its output is NOT the DFT (its "bit-reversal for radix-4" loop,
 * fft.rs:1462-1474, flips one bit per base-4 digit instead of reversing the digits).  A drop-in returns the reference's
 * bytes: the host mirrors' fft_with_strategy(.., Radix4) calls these entries BY DEFAULT (round 6); their radix4_compat =
 * false / KOFFT_HIP_RADIX4_COMPAT=0 opts out and gives the true transform for every strategy, like every other entry
 * point here.  The swap loop runs as a gather through its net permutation, butterfly4 in the reference's operation order,
 * the three running-product twiddle sequences of every stage built on the host with Complex::mul (O(n) host work and
 * 12 / 20 bytes of device tables per point, once per (context, n)).  n not a power of four -> fft() (fft.rs:1457-1460;
 * n == 0 -> EMPTY_INPUT); n > 2^26 -> KOFFT_ERR_UNSUPPORTED (the limit of kofft_hip_fft_*).  data: batch * n complex. */
int kofft_hip_fft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch);
int kofft_hip_fft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch);
int kofft_hip_fft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_fft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch);
/* FftPlan::ifft with strategy Radix4 (fft.rs:2040-2055 -> 2037 -> 1356): `c.im = -c.im`, fft_radix4, `c.im = -c.im;
 * c.re * scale; c.im * scale` with scale = 1 / (n as f32 -> T), the conjugations and the scale folded into the first
 * gather and the last stage's store.  Lengths that are not a power of four: ifft()'s arithmetic (fft.rs:1163-1172). */
int kofft_hip_ifft_radix4_c32(kofft_hip_ctx *ctx, float *data, size_t n, size_t batch);
int kofft_hip_ifft_radix4_c64(kofft_hip_ctx *ctx, double *data, size_t n, size_t batch);
int kofft_hip_ifft_radix4_c32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_ifft_radix4_c64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n, size_t batch);

/* FftImpl::fft_strided / ifft_strided (fft.rs:1175-1199, 1236-1260), host pointers:
 * gathers n = scratch_len elements data[i*stride], transforms, scatters back.
 * stride == 0 -> KOFFT_ERR_INVALID_STRIDE; n == 0 -> KOFFT_OK;
 * data_len < (n-1)*stride+1 -> KOFFT_ERR_MISMATCHED_LENGTHS. */
int kofft_hip_fft_c32_strided(kofft_hip_ctx *ctx, float *data, size_t data_len, size_t stride,
                              size_t n, int inverse);
int kofft_hip_fft_c64_strided(kofft_hip_ctx *ctx, double *data, size_t data_len, size_t stride,
                              size_t n, int inverse);

/* ---- real FFT -----------------------------------------------------------------
 * RfftPlanner::rfft_with_scratch -> rfft_direct (rfft.rs:264-282, 425-465) on `batch`
 * contiguous rows of n reals; out: batch * (n/2+1) complex.  `window` (n reals or
 * NULL) is multiplied into each row first -- the framing product of stft.rs:96.
 * n == 0 -> EMPTY_INPUT; odd n -> INVALID_VALUE.  The reference's scratch argument
 * has no counterpart: the post-pass runs out of LDS.
 * irfft: RfftPlanner::irfft_with_scratch -> irfft_direct (rfft.rs:302-320, 468-508);
 * in: batch * (n/2+1) complex, out: batch * n reals. */
int kofft_hip_rfft_f32(kofft_hip_ctx *ctx, const float *in, float *out, const float *window,
                       size_t n, size_t batch);
int kofft_hip_rfft_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out,
                           const float *d_window, size_t n, size_t batch);
int kofft_hip_irfft_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_irfft_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n,
                            size_t batch);
int kofft_hip_rfft_f64(kofft_hip_ctx *ctx, const double *in, double *out, const double *window,
                       size_t n, size_t batch);
int kofft_hip_rfft_f64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out,
                           const double *d_window, size_t n, size_t batch);
int kofft_hip_irfft_f64(kofft_hip_ctx *ctx, const double *in, double *out, size_t n, size_t batch);
int kofft_hip_irfft_f64_dev(kofft_hip_ctx *ctx, const double *d_in, double *d_out, size_t n,
                            size_t batch);

/* ---- DCT-II -------------------------------------------------------------------
 * DctPlanner::plan_dct2 (dct.rs:16-105), f32 only like the reference, on `batch`
 * contiguous rows of n reals; out: batch * n reals.  Each row is mirrored into 2n
 * reals, rfft_direct'ed (rfft.rs:425-465, inner complex length n) and twisted:
 *   out[k] = 0.5 * (spec[k].re * cos(a_k) + spec[k].im * sin(a_k)),  a_k = PI * k / (2n).
 * The reference's MismatchedLengths (output length != n, dct.rs:68-70) is the
 * caller's to check: both lengths are n here.  batch == 0 -> KOFFT_OK; n == 0 ->
 * EMPTY_INPUT (from the rfft); n beyond the complex transform's range (2^26 for
 * powers of two, 2^25 otherwise) -> KOFFT_ERR_UNSUPPORTED.  _dev: device pointers,
 * asynchronous on the context's stream.  Powers of two 32 .. 4096 run one fused kernel
 * (8-byte aligned input); kofft_hip_set_dct_fused(ctx, 0) sends every length of that
 * context through the composed route instead (mirror, n-point transform, post-pass:
 * the same bytes; A/B measurements and tests).  Same results either way. */
int kofft_hip_dct2_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_dct2_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_set_dct_fused(kofft_hip_ctx *ctx, int on);

/* ---- analytic signal ------------------------------------------------------------
 * hilbert::hilbert_analytic (hilbert.rs:13-47), f32 only like the reference, on `batch`
 * contiguous rows of n reals; out: batch * n complex (2 * batch * n floats, interleaved),
 * 8-byte aligned.  Per row: freq = fft((x, +0)); bins 1 .. n/2-1 get re *= 2, im *= 2,
 * bins n/2+1 .. n-1 become (+0, +0); out = ifft(freq) (conj, fft, conj, * 1/n; n == 1:
 * (x[0], +0)).  Checks, in this order and before the context is touched: batch == 0 ->
 * KOFFT_OK; n == 0 -> EMPTY_INPUT; n not a power of two -> NON_POWER_OF_TWO_NO_STD (the
 * reference rejects it; no Bluestein arm here); n > 2^26 -> KOFFT_ERR_UNSUPPORTED; a null
 * pointer or context -> KOFFT_ERR_NULL.  _dev: device pointers, asynchronous on the
 * context's stream; in and out must not overlap (the composed route uses out as its
 * workspace).  Powers of two 32 .. 4096 run one fused kernel (4-byte aligned input);
 * kofft_hip_set_hilbert_fused(ctx, 0) sends every length of that context through the
 * composed route instead (expand, n-point transform, mask, inverse transform: the same
 * bytes; A/B measurements and tests). */
int kofft_hip_hilbert_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_hilbert_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_set_hilbert_fused(kofft_hip_ctx *ctx, int on);

/* ---- real cepstrum --------------------------------------------------------------
 * cepstrum::real_cepstrum (cepstrum.rs:12-33), f32 only like the reference, on `batch`
 * contiguous rows of n reals; out: batch * n reals, the input's bytes.  Per row: freq =
 * fft((x, +0)); every bin becomes (logf(sqrtf(re * re + im * im) + 1e-12f), +0) with the
 * libm crate's logf; out = the real parts of ifft(freq) (conj, fft, conj, * 1/n; n == 1:
 * the early return).  Checks, in this order and before the context is touched: batch == 0
 * -> KOFFT_OK; n == 0 -> EMPTY_INPUT; n not a power of two -> NON_POWER_OF_TWO_NO_STD (the
 * reference rejects it; no Bluestein arm here); n > 2^26 -> KOFFT_ERR_UNSUPPORTED; a null
 * pointer or context -> KOFFT_ERR_NULL.  _dev: device pointers, asynchronous on the
 * context's stream; in == out is allowed (every route reads a row before it writes it), a
 * partial overlap is undefined.  Powers of two 32 .. 4096 run one fused kernel (4-byte
 * aligned input); kofft_hip_set_cepstrum_fused(ctx, 0) sends every length of that context
 * through the composed route instead (expand, n-point transform, log-magnitude, inverse
 * transform, real parts, through the context's scratch: the same bytes; A/B measurements
 * and tests). */
int kofft_hip_cepstrum_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_cepstrum_f32_dev(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_set_cepstrum_fused(kofft_hip_ctx *ctx, int on);

/* ---- FFT convolution and correlation of rows (overlap-save) ------------------------
 * `rows` contiguous signals x of nx f32 samples, a filter h of nh f32 taps -- one for all rows (filters == 1) or one per row (filters ==
 * rows, rows * nh floats) -- and a power-of-two block >= nh.  With hop = block - nh + 1, full = nx + nh - 1 and nb = ceil(full / hop),
 * every value is a composition of the reference's operations, bit for bit:
 *   H = fft((h[i], +0) zero-padded to block) (fft.rs:1054-1132); flags bit 0 (correlate): the taps in reverse order, h[nh - 1 - i],
 *     so that the result is numpy.correlate(x, h, "full") for real data;
 *   for block b of a row: frame[i] = (x[b * hop - (nh - 1) + i], +0) where that sample exists, (+0, +0) elsewhere; X = fft(frame);
 *   Y[k] = X[k] * H[k], Complex::mul un-fused (num.rs:162-165); y = ifft(Y) (fft.rs:1134-1174: conj, fft, conj, * 1 / block);
 *   full_out[b * hop + j] = y[nh - 1 + j].re for j < hop.
 * out receives full_out[out_first .. out_first + out_len) of every row, dense, out_len floats per row ("full": 0, full; "same":
 * (nh - 1) / 2, nx; "valid": nh - 1, nx - nh + 1); blocks wholly outside that window are not computed.  The result's bits depend on
 * block (the reference's table recurrence makes long transforms less accurate).  block == 0: the library's choice, which
 * kofft_hip_convolve_block(nx, nh, &block) returns without a context (EMPTY_INPUT for nx == 0 or nh == 0).  Checks, in this order and
 * before the context or a device is touched: rows == 0 or out_len == 0 -> KOFFT_OK; nx == 0 or nh == 0 -> EMPTY_INPUT; block not a
 * power of two -> NON_POWER_OF_TWO_NO_STD; block < nh -> MISMATCHED_LENGTHS; filters not 1 or rows -> MISMATCHED_LENGTHS; out_first +
 * out_len > full -> MISMATCHED_LENGTHS; a flag bit other than bit 0 -> INVALID_VALUE; block > 65536 -> KOFFT_ERR_UNSUPPORTED; a null
 * pointer or context -> KOFFT_ERR_NULL.  kofft_hip_convolve_f32: host pointers; kofft_hip_dev_convolve_f32: device pointers,
 * asynchronous on the context's stream; out must not overlap x or h.  Blocks 32 .. 4096 run one fused kernel (4-byte aligned x);
 * kofft_hip_set_convolve_fused(ctx, 0) sends every block of that context through the composed route instead (frames into the
 * context's scratch, transform, multiply, inverse transform, gather: the same bytes; A/B measurements and tests). */
int kofft_hip_convolve_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh,
                           size_t block, unsigned flags, float *out, size_t out_first, size_t out_len);
int kofft_hip_dev_convolve_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                               size_t block, unsigned flags, float *d_out, size_t out_first, size_t out_len);
int kofft_hip_set_convolve_fused(kofft_hip_ctx *ctx, int on);
int kofft_hip_convolve_block(size_t nx, size_t nh, size_t *block);

/* ---- filter-bank convolution and correlation of rows (overlap-save) ------------------------
 * The convolution above with `filters` filters of nh taps that every row shares: each frame is loaded and transformed once, then
 * multiplied and transformed back once per filter (filters + 1 transforms per frame where `filters` calls above cost 2 * filters).
 * block, hop, full, nb and the frame are the ones above.  For row r, filter f and block b:
 *   H_f = fft((re, im) of tap i, zero-padded to block).  Real taps: (h[f][i], +0), h holds filters * nh floats.  flags bit 1 (complex
 *     taps): h holds filters * nh interleaved (re, im) f32 pairs.  flags bit 0 (correlate): the taps reversed, complex taps conjugated
 *     as well, conj(h[f][nh - 1 - i]), so that the result is numpy.correlate(x, h_f, "full");
 *   X = fft(frame), once per (row, block);  Y_f[k] = X[k] * H_f[k], Complex::mul un-fused (num.rs:162-165);
 *   y_f = ifft(Y_f) (fft.rs:1134-1174): re = v.re * (1 / block), im = (-v.im) * (1 / block);
 *   element b * hop + j of (row, filter), j < hop, comes from y_f[nh - 1 + j] by the output kind in flags bits 2-3: 0 the real part
 *     (f32), 1 the complex value (an (re, im) f32 pair), 2 the magnitude sqrtf(re * re + im * im) of the scaled values (the sum
 *     un-fused, the root correctly rounded).
 * out is dense [rows][filters][out_len] elements of 4 bytes (kinds 0 and 2) or 8 bytes (kind 1), aligned to its element, and holds
 * full_out[out_first .. out_first + out_len) of every (row, filter); blocks wholly outside that window are not computed.  With real
 * taps and kind 0, (row, filter) has the bits kofft_hip_convolve_f32 gives for that filter alone.  block == 0: kofft_hip_convolve_block(nx,
 * nh).  Checks, in this order and before the context or a device is touched: rows == 0, filters == 0 or out_len == 0 -> KOFFT_OK;
 * nx == 0 or nh == 0 -> EMPTY_INPUT; block not a power of two -> NON_POWER_OF_TWO_NO_STD; block < nh -> MISMATCHED_LENGTHS; out_first +
 * out_len > full -> MISMATCHED_LENGTHS; a flag bit above bit 3, or output kind 3 -> INVALID_VALUE; block > 65536 ->
 * KOFFT_ERR_UNSUPPORTED; a null pointer or context -> KOFFT_ERR_NULL.  kofft_hip_convolve_bank_f32: host pointers;
 * kofft_hip_dev_convolve_bank_f32: device pointers, asynchronous on the context's stream; out must not overlap x or h.  Blocks 32 ..
 * 4096 run one fused kernel (4-byte aligned x); kofft_hip_set_convolve_bank_fused(ctx, 0) sends every block of that context through
 * the composed route instead (frames into the context's scratch and transformed once, then per filter multiply, inverse transform,
 * gather: the same bytes; A/B measurements and tests). */
#define KOFFT_HIP_BANK_CORRELATE 1u
#define KOFFT_HIP_BANK_COMPLEX_TAPS 2u
#define KOFFT_HIP_BANK_OUT_REAL 0u
#define KOFFT_HIP_BANK_OUT_COMPLEX 4u
#define KOFFT_HIP_BANK_OUT_MAGNITUDE 8u
int kofft_hip_convolve_bank_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t filters, size_t nh,
                                size_t block, unsigned flags, void *out, size_t out_first, size_t out_len);
int kofft_hip_dev_convolve_bank_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t filters, size_t nh,
                                    size_t block, unsigned flags, void *d_out, size_t out_first, size_t out_len);
int kofft_hip_set_convolve_bank_fused(kofft_hip_ctx *ctx, int on);

/* ---- fast DCT-IV of rows, MDCT of rows of signals and IMDCT ------------------------
 * f32 only.  The reference has no such entry point; every value is a composition of its operations, all arithmetic f32 and un-fused,
 * met bit for bit by every route.  "fft" is the reference's fft (fft.rs:1054-1132): a length that is not a power of two goes through
 * its Bluestein arm.
 * Tables.  kofft_hip_dct4_table_f32(n, out), n even, M = n / 2, needs no context or device: it writes M pairs c[j] = (cos a_j, sin a_j),
 *   a_j = -PI (4j + 1) / (4n), then M pairs d[k] = (cos b_k, sin b_k), b_k = -PI k / n (2n floats); every angle and every cos / sin is
 *   computed in double and rounded once to f32.  n == 0 -> EMPTY_INPUT; n odd -> INVALID_VALUE; out null -> KOFFT_ERR_NULL.
 * dct4_fast(u), N even, M = N / 2:
 *   z[j] = (u[2j], u[N-1-2j]) * c[j] for j < M, Complex::mul (num.rs:162-165: four products, one subtract, one add);
 *   Z = fft(z) (nothing for M == 1);  y[k] = Z[k] * d[k];  X[2k] = y[k].re and X[N-1-2k] = -y[k].im.
 *   In exact arithmetic X[k] = sum_i u[i] cos(PI / N (i + 1/2)(k + 1/2)): dct::dct4 without its O(n^2) loop.  The two differ in the
 *   last bits; kofft_hip_dct4_f32 stays the direct sum.
 *   kofft_hip_dct4_fast_f32 / kofft_hip_dev_dct4_fast_f32: batch rows of n reals in, batch rows of n reals out; out may equal in, no
 *   other overlap.  Checks, in this order and before the context or a device is touched: batch == 0 -> KOFFT_OK; n == 0 ->
 *   EMPTY_INPUT; n odd -> INVALID_VALUE; n / 2 beyond the complex limits (2^26 for powers of two, 2^25 otherwise) or batch * n too
 *   large -> KOFFT_ERR_UNSUPPORTED; a null pointer or context -> KOFFT_ERR_NULL.
 * MDCT.  `rows` signals of nx samples, row r at x + r * row_stride (in floats; ignored when rows == 1), a window w of 2N values,
 *   `frames` frames per row, `lead` < 2N virtual zeros in front of every row.  Frame f, for i < 2N:
 *     g[i] = x[f N + i - lead] * w[i] where that sample exists in its own row, +0 elsewhere (never a sample of row r +- 1);
 *     u[j] = (-g[3N/2-1-j]) - g[3N/2+j] for j < N/2;  u[j] = g[j-N/2] - g[3N/2-1-j] for N/2 <= j < N;
 *   the coefficients of frame (r, f) are dct4_fast(u), dense at out[(r * frames + f) * N].  In exact arithmetic
 *   X[k] = sum_{i < 2N} g[i] cos(PI / N (i + 1/2 + N/2)(k + 1/2)), unscaled.  out must not overlap x or w.
 *   Checks, in this order: rows == 0 or frames == 0 -> KOFFT_OK; N == 0 -> EMPTY_INPUT; N odd -> INVALID_VALUE; N / 2 beyond the
 *   complex limits -> KOFFT_ERR_UNSUPPORTED; nx == 0 -> EMPTY_INPUT; lead >= 2N -> INVALID_VALUE; rows > 1 and row_stride < nx ->
 *   INVALID_VALUE; sizes that overflow -> KOFFT_ERR_UNSUPPORTED; a null pointer or context -> KOFFT_ERR_NULL.
 * IMDCT.  coef is rows * frames * N coefficients, w a window of 2N values.  v_f = dct4_fast(X_f);
 *     y_f[i] = v[N/2+i] for i < N/2;  -v[3N/2-1-i] for N/2 <= i < 3N/2;  -v[i-3N/2] for 3N/2 <= i < 2N.
 *   Each row has full = (frames + 1) N samples in hop blocks b of N: where both frames exist,
 *     full[b N + j] = (w[N+j] * y_{b-1}[N+j] + w[j] * y_b[j]) * scale, the earlier frame's term on the left;
 *   in blocks 0 and `frames` only one term exists and the value is that product * scale.  out receives full[out_first .. out_first +
 *   out_len) of every row, dense, out_len floats per row.  With a Princen-Bradley window (w[i]^2 + w[i+N]^2 = 1), lead = N, scale =
 *   2 / N, out_first = N and out_len = nx the result is the signal wherever two frames cover a sample.  out must not overlap coef or w.
 *   Checks, in this order: rows == 0, frames == 0 or out_len == 0 -> KOFFT_OK; N == 0 -> EMPTY_INPUT; N odd -> INVALID_VALUE; N / 2
 *   beyond the complex limits or sizes that overflow -> KOFFT_ERR_UNSUPPORTED; out_first + out_len > full -> MISMATCHED_LENGTHS; a
 *   null pointer or context -> KOFFT_ERR_NULL.
 * The host forms stage through the context's buffers; the kofft_hip_dev_* forms take device pointers and are asynchronous on the
 * context's stream.  N = 64 .. 8192 a power of two with 4-byte aligned inputs runs one fused kernel per DCT-IV (the MDCT's window
 * and fold on its loads); every other N, and every N after kofft_hip_set_mdct_fused(ctx, 0), runs the composed route through the
 * context's scratch (fold / pre-twiddle, transform, post-twiddle: the same bytes; A/B measurements and tests).  The IMDCT writes the
 * frames' DCT-IV into scratch the context owns (until kofft_hip_release_scratch / destroy), then one unfold-window-add kernel. */
int kofft_hip_dct4_table_f32(size_t n, float *out);
int kofft_hip_dct4_fast_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_dev_dct4_fast_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_mdct_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, size_t row_stride, const float *window, size_t n,
                       size_t lead, float *out, size_t frames);
int kofft_hip_dev_mdct_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, size_t row_stride, const float *d_window, size_t n,
                           size_t lead, float *d_out, size_t frames);
int kofft_hip_imdct_f32(kofft_hip_ctx *ctx, const float *coef, size_t rows, size_t frames, const float *window, size_t n, float scale,
                        float *out, size_t out_first, size_t out_len);
int kofft_hip_dev_imdct_f32(kofft_hip_ctx *ctx, const float *d_coef, size_t rows, size_t frames, const float *d_window, size_t n, float scale,
                            float *d_out, size_t out_first, size_t out_len);
int kofft_hip_set_mdct_fused(kofft_hip_ctx *ctx, int on);

/* ---- polyphase filter bank of rows: analysis and synthesis (weighted overlap-add) -----------------
 * A prototype filter of nh = T M taps folded onto an M-point transform: M channels, T >= 1 taps per channel, hop D >= 1, h the nh
 * analysis taps, g the nh synthesis taps.  f32 only; one filter for all rows.  The reference has no such entry point: "fft" and "ifft"
 * below are its own (fft.rs), exactly as kofft_hip_stft_rows_f32 and kofft_hip_istft_parallel_rows_f32 use them, the Bluestein arm for
 * lengths that are not a power of two and ifft as conj, fft, conj, * 1 / M included.  Every route, grid and device meets the
 * definitions bit for bit; all arithmetic is f32 and un-fused: one product, then one sum.
 * Analysis.  `rows` signals of nx samples, row r at x + r * row_stride (in floats; ignored when rows == 1), `lead` < nh virtual zeros
 *   in front of every row, `frames` frames per row (the caller's; frames past the end read +0).  Item (r, f), for j < M and t < T:
 *     g_t  = h[j + tM] * x_r[fD + j + tM - lead]   where that sample exists in its own row, +0 elsewhere (never a sample of row r +- 1);
 *     u[j] = (..((g_0 + g_1) + g_2)..) + g_{T-1}   ascending t, one accumulator started by g_0;
 *     Z    = fft((u[j], +0))                       (nothing for M == 1);
 *     out[(r * frames + f) * bins + k] = Z[k], k < bins: complex, dense, 8-byte aligned.
 *   1 <= bins <= M; bins = M / 2 + 1 is the one-sided form.  Nothing of the other bins is written anywhere.  In exact arithmetic
 *   Z[k] = sum_{i < nh} h[i] x[fD + i - lead] exp(-2 PI i k i / M).  With T = 1 and lead = 0 this is kofft_hip_stft_rows_f32 with window
 *   h and hop D.  out must not overlap x or h.
 *   Checks, in this order and before the context or a device is touched: rows == 0 or frames == 0 -> KOFFT_OK, nothing touched;
 *   M == 0 or nh == 0 -> EMPTY_INPUT; nh % M != 0, or bins == 0 or bins > M -> INVALID_VALUE; M beyond the complex limits (2^26 for
 *   powers of two, 2^25 otherwise) -> KOFFT_ERR_UNSUPPORTED; D == 0 -> INVALID_HOP_SIZE; nx == 0 -> EMPTY_INPUT; lead >= nh ->
 *   INVALID_VALUE; rows > 1 and row_stride < nx -> INVALID_VALUE; sizes that overflow -> KOFFT_ERR_UNSUPPORTED; a null pointer or
 *   context -> KOFFT_ERR_NULL.
 * Synthesis.  spec is rows * frames * bins complex (8-byte aligned) and is only read.  bins == M: the frames are used as given;
 *   bins == M / 2 + 1 with M even: completed as kofft_hip_istft_onesided_f32 does, F[k] = (half[M-k].re, -half[M-k].im) for
 *   k >= bins, the imaginary parts of bins 0 and M / 2 used as given; any other bins -> INVALID_VALUE.  Per frame and row:
 *     v_f = ifft(F_f);  r_f[j] = v_f[j].re;  full = (frames - 1) D + nh samples per row;
 *     full[p] = (sum over f ascending with 0 <= p - fD < nh of g[p - fD] * r_f[(p - fD) mod M]) * scale,
 *   the first term starting the accumulator; a sample no frame covers is +0.  out receives full[out_first .. out_first + out_len) of
 *   every row, dense, out_len floats per row.  out must not overlap spec or g.
 *   Checks: the analysis ones that apply, in their order -- rows == 0 or frames == 0 -> KOFFT_OK; M == 0 or nh == 0 -> EMPTY_INPUT;
 *   nh % M != 0 or a bins that is neither form -> INVALID_VALUE; M beyond the complex limits -> KOFFT_ERR_UNSUPPORTED; D == 0 ->
 *   INVALID_HOP_SIZE; sizes that overflow -> KOFFT_ERR_UNSUPPORTED --, then out_first + out_len > full -> MISMATCHED_LENGTHS; a null
 *   pointer or context -> KOFFT_ERR_NULL (out may be null when out_len == 0, which writes nothing).
 *   Reconstruction is exact when, for every p mod D, sum_f g[n_f] * h[n_f + qM] = c * delta[q] with n_f = p - fD: the round trip then
 *   needs lead = nh - D, out_first = lead and scale = 1 / c, and returns x wherever every covering frame exists.  The sine window
 *   with T = 1 and D = M / 2 is such a pair (c = 1); a sinc x Kaiser prototype used as h = g is not.
 * Host helpers, no context, no device, everything in double and rounded to f32 once where the result is f32.
 *   kofft_hip_pfb_taps_f32(M, T, beta, out) writes the nh = T M values sinc((i - (nh - 1) / 2) / M) * Kaiser_beta[i], normalised to unit
 *   sum (sinc(t) = sin(PI t) / (PI t); Kaiser_beta[i] = I0(beta sqrt(1 - (2i / (nh - 1) - 1)^2)) / I0(beta), I0 the power series of
 *   kofft_hip_resample_taps_f32).  M == 0 or T == 0 -> EMPTY_INPUT; beta < 0 or NaN -> INVALID_VALUE; out null -> KOFFT_ERR_NULL; more
 *   than 2^28 taps -> KOFFT_ERR_UNSUPPORTED.
 *   kofft_hip_pfb_reconstruction(h, g, nh, M, D, &c, &worst) evaluates the condition above in double: *c is the q = 0 sum at p = 0,
 *   *worst the largest |sum - c * delta[q]| over all p mod D and |q| < T.  M == 0 or nh == 0 -> EMPTY_INPUT; nh % M != 0 ->
 *   INVALID_VALUE; D == 0 -> INVALID_HOP_SIZE; a null pointer -> KOFFT_ERR_NULL.
 * The host forms stage through the context's buffers; the kofft_hip_dev_* forms take device pointers and are asynchronous on the
 * context's stream.  Routes, the same bytes.  The fused kernels exist for M = 32 .. 4096 a power of two with 4-byte aligned x and h: one per
 * analysis (fold on its loads, the kept bins on its stores) and one per chunk of inverse transforms.  The composed route takes every
 * M through scratch the context owns (fold, transform, prefix copy; completion, inverse transform, real parts).  The synthesis then
 * runs one overlap-add kernel, one thread per sample.  kofft_hip_set_pfb_fused(ctx, on): 1, the default, the measured choice (DESIGN
 * 5.34: the fused analysis up to M = 1024, the fused inverse wherever it exists); 0 every call of the context through the composed
 * route; 2 the fused kernels wherever they exist (A/B measurements and tests); anything else -> INVALID_VALUE. */
int kofft_hip_pfb_analysis_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, size_t row_stride, const float *h, size_t nh, size_t m,
                               size_t d, size_t lead, float *out, size_t frames, size_t bins);
int kofft_hip_dev_pfb_analysis_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, size_t row_stride, const float *d_h, size_t nh,
                                   size_t m, size_t d, size_t lead, float *d_out, size_t frames, size_t bins);
int kofft_hip_pfb_synthesis_f32(kofft_hip_ctx *ctx, const float *spec, size_t rows, size_t frames, size_t bins, const float *g, size_t nh, size_t m,
                                size_t d, float scale, float *out, size_t out_first, size_t out_len);
int kofft_hip_dev_pfb_synthesis_f32(kofft_hip_ctx *ctx, const float *d_spec, size_t rows, size_t frames, size_t bins, const float *d_g, size_t nh,
                                    size_t m, size_t d, float scale, float *d_out, size_t out_first, size_t out_len);
int kofft_hip_pfb_taps_f32(size_t m, size_t taps, double beta, float *out);
int kofft_hip_pfb_reconstruction(const float *h, const float *g, size_t nh, size_t m, size_t d, double *c, double *worst);
int kofft_hip_set_pfb_fused(kofft_hip_ctx *ctx, int on);

/* ---- polyphase resampling of rows (upfirdn, resample_poly) -----------------------------------
 * Sample-rate conversion by up / down of `rows` dense rows of nx f32 samples through one FIR filter of nh taps: out_len values per row
 * from up-sampled time t0 on, the decimating or interpolating filter computed directly in the time domain (with up == down == 1 a
 * plain FIR).  f32 only; one filter for all rows; no gcd reduction: up and down are used as given.
 * Definition, met bit for bit by every route, grid and device.  Let xu be x with up - 1 zeros after every sample (xu[i * up] = x[i]);
 * the full filtered length is full_up = (nx - 1) * up + nh.  Output m of a row sits at up-sampled time t = t0 + m * down:
 *   p = t mod up;  i0 = t div up;  acc = +0.0f
 *   for j = 0, 1, 2, .. while p + j * up < nh:       (ascending j, one accumulator)
 *       i = i0 - j;  if 0 <= i < nx:  acc = acc + (h[p + j * up] * x[i])      (one f32 product, then one f32 sum: never fused)
 *   out[m] = acc
 * Terms whose sample does not exist are skipped, not multiplied by zero: a NaN or Inf of x reaches exactly the outputs whose term set
 * holds it, and an output without terms is +0.  All position arithmetic (t, i0, p + j * up) is 64-bit.
 * This is scipy.signal.upfirdn(h, x, up, down) for t0 = 0 and out_len = ceil(full_up / down), and scipy.signal.resample_poly's
 * alignment (the taps already multiplied by up) for t0 = (nh - 1) / 2 and out_len = ceil(nx * up / down).
 * Checks, in this order and before the context or a device is touched: rows == 0 or out_len == 0 -> KOFFT_OK, nothing touched;
 * nx == 0 or nh == 0 -> EMPTY_INPUT; up == 0 or down == 0 -> INVALID_VALUE; full_up, t0 + (out_len - 1) * down or a byte count
 * beyond 64 bits -> KOFFT_ERR_UNSUPPORTED; t0 + (out_len - 1) * down >= full_up (an output wholly past the result) ->
 * MISMATCHED_LENGTHS; a null pointer or context -> KOFFT_ERR_NULL; out overlapping x or h -> INVALID_VALUE.
 * Routes, the same bytes.  The plain kernel takes every shape: one thread per output, samples and taps from global memory.  The tiled
 * kernel gives a 256-thread workgroup up to KOFFT_HIP_RESAMPLE_TILE consecutive outputs of one row at a time: the samples their terms name
 * and the taps in phase-major order lie in LDS, one pass over HBM; it exists where both fit 52 KiB.  kofft_hip_set_resample_tiled(ctx,
 * on): 1, the default, the measured choice; 0 every call of the context on the plain kernel; 2 the tiled kernel
 * wherever its tables fit (A/B measurements and tests); anything else -> INVALID_VALUE.  kofft_hip_resample_route, no context: *route = 1 where a default context runs the tiled kernel, 0 where the plain one; for
 * fixed up and down it is 1 up to some nh and 0 beyond.  nh == 0 -> EMPTY_INPUT, up == 0 or down == 0 -> INVALID_VALUE, route null ->
 * KOFFT_ERR_NULL.  kofft_hip_dev_resample_f32 takes device pointers and is asynchronous on the context's stream.
 * kofft_hip_resample_taps_f32, host only, no context: what scipy.signal.resample_poly designs by default (zeros = 10, beta = 5.0).
 * half = zeros * max(up, down), *nh = 2 * half + 1; the sinc of cutoff 1 / max(up, down) under a Kaiser window of `beta`, normalised to
 * unit sum, times up; everything in double (I0 by its power series), rounded to f32 once.  taps == NULL: *nh alone.  taps and nh both
 * null -> KOFFT_ERR_NULL; up, down or zeros == 0, beta < 0 or NaN -> INVALID_VALUE; a length beyond 2^28 taps -> KOFFT_ERR_UNSUPPORTED.
 * The device contract never depends on this helper: the taps are an input, as the mel edges are. */
#define KOFFT_HIP_RESAMPLE_TILE 1024
int kofft_hip_resample_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *h, size_t nh, size_t up, size_t down,
                           size_t t0, float *out, size_t out_len);
int kofft_hip_dev_resample_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_h, size_t nh, size_t up,
                               size_t down, size_t t0, float *d_out, size_t out_len);
int kofft_hip_set_resample_tiled(kofft_hip_ctx *ctx, int on);
int kofft_hip_resample_route(size_t nh, size_t up, size_t down, int *route);
int kofft_hip_resample_taps_f32(size_t up, size_t down, size_t zeros, double beta, float *taps, size_t *nh);

/* ---- IIR filtering of rows by a cascade of biquads (sosfilt) -----------------------------------
 * scipy.signal.sosfilt on `rows` dense rows of nx f32 samples: `sections` >= 1 second-order sections sos[sections][6] =
 * b0 b1 b2 a0 a1 a2 (scipy's layout), one cascade for all rows.  f32 only.  zi[rows][sections][2]: the initial state of every row
 * and section, null for all +0; zf[rows][sections][2]: the final state, null for not stored.  The state is row-major so that batches
 * can be cut by rows (scipy's is [sections][rows][2]; the Python wrapper transposes).  flags: bit 0 KOFFT_HIP_SOSFILT_REVERSE, the
 * row is walked from its last sample to its first (the filter of the flipped row, flipped back; zi / zf are then the state before
 * sample nx - 1 / after sample 0).
 * Definition, met bit for bit by every route, grid and device.  Per row and per section s in ascending s, the section's input v is
 * the previous section's output (x for s = 0); with the section's state (z0, z1), for t = 0 .. nx - 1 (nx - 1 .. 0 with the flag):
 *   y  = (b0 * v[t]) + z0
 *   z0 = ((b1 * v[t]) - (a1 * y)) + z1
 *   z1 = (b2 * v[t]) - (a2 * y)
 *   out[t] = y
 * Every product and every sum is one rounded f32 operation in exactly this association (never fused; f32 subnormals are kept); NaN
 * and Inf propagate as the recurrence says.  The nesting of the loops over sections and samples is not part of the contract: either
 * order gives the same bits.  a0 is not divided by: it must be 1.0f, as scipy demands.  A rounded recurrence cannot be cut along
 * time without changing bits: a row is walked sequentially and the parallelism is across rows.
 * Checks, in this order and before the context or a device is touched: rows == 0 or nx == 0 -> KOFFT_OK, nothing touched (zf is not
 * written either); sections == 0 -> EMPTY_INPUT; an unknown flag bit -> INVALID_VALUE; a byte count beyond 64 bits ->
 * KOFFT_ERR_UNSUPPORTED; x, sos, out or the context null -> KOFFT_ERR_NULL; out overlapping x other than out == x exactly, or zf
 * overlapping zi other than zf == zi exactly -> INVALID_VALUE; an output (out, zf) overlapping sos, the other output, or the input
 * that is not its own (zf over x, out over zi) -> INVALID_VALUE; host form only, where sos can be read: some a0 != 1.0f ->
 * INVALID_VALUE (the device form requires it and does not read device memory to check).  Filtering in place (out == x, zf == zi) is
 * allowed.
 * Routes, the same bytes.  The plain kernel: one thread per row walks its row in global memory.  The tiled kernel: a wavefront owns 64
 * rows and walks them in tiles of KOFFT_HIP_SOSFILT_TILE samples staged through LDS with coalesced loads and stores.  Either holds
 * at most KOFFT_HIP_SOSFILT_GROUP sections per pass; a longer cascade runs further passes in place over out.
 * kofft_hip_set_sosfilt_tiled(ctx, on): 1, the default, the measured choice; 0 every call of the context on the plain
 * kernel; 2 the tiled kernel wherever it exists (A/B measurements and tests); anything else -> INVALID_VALUE.
 * kofft_hip_sosfilt_route, no context: *route = 1 where a default context runs the tiled kernel, 0 where the plain one; the measured
 * rule depends on `rows` alone (the tiled kernel from 16 rows on).  route null -> KOFFT_ERR_NULL.
 * kofft_hip_dev_sosfilt_f32 takes device pointers and is asynchronous on the context's stream. */
#define KOFFT_HIP_SOSFILT_REVERSE 1u
#define KOFFT_HIP_SOSFILT_TILE 32
#define KOFFT_HIP_SOSFILT_GROUP 8
int kofft_hip_sosfilt_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                          float *zf, unsigned flags, float *out);
int kofft_hip_dev_sosfilt_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                              const float *d_zi, float *d_zf, unsigned flags, float *d_out);
int kofft_hip_set_sosfilt_tiled(kofft_hip_ctx *ctx, int on);
int kofft_hip_sosfilt_route(size_t rows, int *route);

/* ---- the same cascade as a scan along time (sosfilt_scan) ---------------------------------------
 * kofft_hip_sosfilt_f32 walks a row sequentially; few long rows leave the device idle.  kofft_hip_sosfilt_scan_f32 takes the same
 * arguments plus `chunk`, cuts every row into chunks of `chunk` samples and filters all chunks of all rows in parallel.  It has its
 * own bit-exact definition: the same recurrence inside a chunk, but the state at a seam is computed, not walked, so the bits differ
 * from kofft_hip_sosfilt_f32's after the first chunk (by the rounding of an f32 recurrence: DESIGN 5.30 has the accuracy table).
 * Definition, met bit for bit by every batch size, grid and entry point.  The cascade runs in groups of KOFFT_HIP_SOSFILT_GROUP
 * sections; group g filters the output of group g - 1.  For one group of S sections: D = 2 S, component i = 2 s + k of a state vector
 * is z_k of section s; C = ceil(nx / chunk); chunk c holds samples [c * chunk, min(nx, (c + 1) * chunk)); "the walk" is the
 * recurrence of kofft_hip_sosfilt_f32, every product and sum one rounded f32 operation, never fused, subnormals kept.
 *   1. M[i][j] is component i of the group's state after walking `chunk` samples of +0.0f from the state e_j (component j 1.0f, the
 *      others +0.0f); the walk is followed literally, b * 0 terms included.
 *   2. p_c, c = 0 .. C - 2, is the group's state after walking chunk c from the all +0 state.
 *   3. Z_0 is the row's zi (all +0 without one).  For c = 0 .. C - 2 and every i, with J = 2 * (i / 2) + 2:
 *        Z_{c+1}[i] = ((((M[i][0] * Z_c[0]) + (M[i][1] * Z_c[1])) + ...) + (M[i][J-1] * Z_c[J-1])) + p_c[i]
 *      in ascending j, every product and sum one rounded f32 operation.  Only the columns of the sections <= i / 2 enter: the others
 *      are exact zeros of M, and leaving them out keeps an Inf in a later section's state from making an earlier component NaN.
 *   4. Chunk c of out is the walk of chunk c from Z_c; zf is the state at the end of the walk of chunk C - 1.
 * With C == 1 the bytes are kofft_hip_sosfilt_f32's, and chunk 0 of any call equals its first `chunk` samples.  With
 * KOFFT_HIP_SOSFILT_REVERSE the result is the forward definition applied to the time-reversed row: chunk c holds samples
 * [max(0, nx - (c + 1) * chunk), nx - c * chunk), walked downwards; the short chunk is the last in walk order in both directions.
 * `chunk` is part of the contract: another chunk gives other bits.  Cutting a row into two calls (zf -> zi) is correct to the same
 * accuracy but not bit-identical to one call: the seam state of one call is M Z + p, not a walked state.
 * Checks: those of kofft_hip_sosfilt_f32 in its order, with one added directly after the flag check -- chunk == 0 or not a multiple
 * of KOFFT_HIP_SOSFILT_TILE -> INVALID_VALUE -- and the byte count of the state scratch added to the 64-bit overflow checks
 * (KOFFT_ERR_UNSUPPORTED).  In place (out == x, zf == zi) is allowed: the walk that stores zf takes every chunk's initial state from the
 * scratch, where an earlier launch has copied zi, so no launch reads zi while another part of it writes zf.  The host form checks a0 == 1.0f; the device form requires it.
 * Three launches per group: a walk of all chunks from +0 that keeps only the final states (and M, from 2 S further walks of zeros),
 * a sequential carry over the C - 1 seams of every row, a walk of all chunks from their true states that stores out.  The states,
 * rows * C * D floats, live in the context's scratch; a batch whose states exceed KOFFT_HIP_SCRATCH_CHUNK_MB goes in pieces of
 * whole rows.  Two reads and one write of every sample instead of one and one; faster than kofft_hip_sosfilt_f32 on few long rows,
 * slower on many short ones (DESIGN 5.30 says where).
 * kofft_hip_sosfilt_scan_chunk, no context: *chunk = the measured choice for the shape, never below 1024 (shorter chunks are legal
 * but cost accuracy where poles lie within ~1e-3 of the unit circle).  chunk null -> KOFFT_ERR_NULL.
 * kofft_hip_dev_sosfilt_scan_f32 takes device pointers and is asynchronous on the context's stream. */
int kofft_hip_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *x, size_t rows, size_t nx, const float *sos, size_t sections, const float *zi,
                               float *zf, size_t chunk, unsigned flags, float *out);
int kofft_hip_dev_sosfilt_scan_f32(kofft_hip_ctx *ctx, const float *d_x, size_t rows, size_t nx, const float *d_sos, size_t sections,
                                   const float *d_zi, float *d_zf, size_t chunk, unsigned flags, float *d_out);
int kofft_hip_sosfilt_scan_chunk(size_t rows, size_t nx, size_t sections, size_t *chunk);

/* ---- Welch power spectra and cross spectra of rows ------------------------------------------
 * The sum over frames of |X[k]|^2 (welch) or conj(X[k]) Y[k] (csd) of `rows` signals of `len` f32 samples, row r at signal + r *
 * row_stride, `frames` frames per row; no frame ever reaches the caller.  psd is rows * K floats, pxy rows * K interleaved complex,
 * K = win_len / 2 + 1.  f32 only.  There is no detrending and no median.
 * Arithmetic contract, met bit for bit by every route, grid, chunk size and device:
 *   Frames and bins.  Frame f of row r has the spectrum X[k], k < K, that kofft_hip_stft_onesided_f32 writes for it: the same window
 *     product, +0 past the end of the row and never the head of row r + 1, the reference's FFT or its Bluestein arm, every win_len that
 *     call takes.  window == NULL: window::hann(win_len), as in kofft_hip_stft_mel_f32.  csd: X and Y are the spectra of frame f of row
 *     r of x and of y, two signals with the same len, row_stride, window and hop.
 *   Per frame and bin, nothing fused.  welch: p = re * re + im * im.  csd: c.re = xr * yr + xi * yi, c.im = xr * yi - xi * yr
 *     (conj(X) Y, scipy.signal.csd's sign).
 *   Summation order.  The frames of a row are cut into groups of KOFFT_HIP_WELCH_GROUP = 32 consecutive frames counted from frame 0
 *     of that row; the last group is shorter when 32 does not divide `frames`.  A group's partial is the f32 sum of its frames' values
 *     in ascending frame order, seeded with +0.  The row's total is the f32 sum of its partials in ascending group order, seeded with
 *     +0.  No atomics, no trees.
 *   Output.  out[k] = total[k] * scale, one f32 multiplication (csd: both parts).  With KOFFT_HIP_PSD_DOUBLE in flags the interior
 *     bins are then multiplied by 2.0f: (total * scale) * 2.0f.  Interior: 1 <= k < K - 1 for even win_len, 1 <= k < K for odd.
 * `frames` is the caller's and has no lower bound (kofft_amd.psd passes the number of whole segments); frames wholly past the row
 * contribute +0.  Checks, in this order and before the context or the device is touched: hop == 0 -> INVALID_HOP_SIZE; rows == 0 or
 * frames == 0 -> KOFFT_OK, nothing touched; win_len == 0 -> EMPTY_INPUT; win_len beyond the complex limits (kofft_hip_stft_rows_f32's)
 * -> UNSUPPORTED; rows > 1 and row_stride < len -> INVALID_VALUE; sizes that overflow -> UNSUPPORTED; then a flag bit other than
 * KOFFT_HIP_PSD_DOUBLE -> INVALID_VALUE; a null data pointer (a signal with len > 0, the output) or a null context -> KOFFT_ERR_NULL;
 * the output overlapping a signal or the window -> INVALID_VALUE.
 * Routes, the same bytes.  The fused kernel (power-of-two win_len 64 .. 4096) gives a group of frames to a slot of threads that keeps
 * the running sums of its bins in registers while it walks the frames through LDS; rows of more than one group leave their partials
 * in the context's scratch for a second small kernel.  The composed route (every other win_len, Bluestein lengths such as 400 too)
 * writes the one-sided frames of whole groups into the context's scratch (KOFFT_HIP_SCRATCH_CHUNK_MB at a time) and sums them there.
 * kofft_hip_set_welch_fused(ctx, mode): 1, the default, the measured choice; 0 every call composed; 2 the fused kernel
 * wherever it exists (A/B measurements and tests); anything else -> INVALID_VALUE.  The kofft_hip_dev_* forms take device pointers and
 * are asynchronous on the context's stream (named so for the reason given at the chirp-Z entries; their guard-band cases live in
 * tests/test_gpu_welch_footprint.py).
 * kofft_hip_welch_scale_f32, host only, no context: scaling 0 (density) 1 / (fs * sum w[i]^2 * frames), scaling 1 (spectrum) 1 /
 * ((sum w[i])^2 * frames); the sums ascending in double over the f32 window (NULL: window::hann(win_len)), the result rounded to f32
 * once.  scale null -> KOFFT_ERR_NULL; win_len == 0 -> EMPTY_INPUT; another scaling, fs <= 0 (or NaN), frames == 0 or a zero sum ->
 * INVALID_VALUE.  Coherence and transfer functions are compositions: |csd(x, y)|^2 / (welch(x) welch(y)) and csd(x, y) / welch(x). */
#define KOFFT_HIP_WELCH_GROUP 32
#define KOFFT_HIP_PSD_DOUBLE 1
int kofft_hip_welch_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                        size_t win_len, size_t hop, size_t frames, float scale, int flags, float *psd);
int kofft_hip_dev_welch_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window,
                            size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_psd);
int kofft_hip_csd_f32(kofft_hip_ctx *ctx, const float *x, const float *y, size_t rows, size_t len, size_t row_stride, const float *window,
                      size_t win_len, size_t hop, size_t frames, float scale, int flags, float *pxy);
int kofft_hip_dev_csd_f32(kofft_hip_ctx *ctx, const float *d_x, const float *d_y, size_t rows, size_t len, size_t row_stride,
                          const float *d_window, size_t win_len, size_t hop, size_t frames, float scale, int flags, float *d_pxy);
int kofft_hip_set_welch_fused(kofft_hip_ctx *ctx, int mode);
int kofft_hip_welch_scale_f32(const float *window, size_t win_len, double fs, size_t frames, int scaling, float *scale);

/* ---- mel filterbank and MFCC ------------------------------------------------------
 * cepstrum::mel_filterbank / mfcc / mfcc_batch (cepstrum.rs:36-98), f32 only like the reference, on `rows` contiguous rows of n_fft
 * magnitudes -- what kofft_hip_dev_stft_magnitudes_rows_f32 writes, rows x frames flattened.  The filter edges are an INPUT: bins is
 * a HOST pointer (in both forms) to num_mel + 2 nondecreasing values, read before the call returns.  Everything after the edges is
 * the reference's arithmetic bit for bit, all f32, never fused:
 *   energies (rows x num_mel): filter m has a = bins[m], b = bins[m + 1], c = bins[m + 2].  b == a or c == b: +0 (the reference's
 *     `continue`).  Otherwise e = +0, then e += ((k - a) as f32 / (b - a) as f32) * x[k] for k = a .. b - 1 and e += ((c - k) as f32 /
 *     (c - b) as f32) * x[k] for k = b .. c - 1, in that order; terms with k >= n_fft are skipped, their edges still set the
 *     denominators; the integer conversions round to nearest, the division is correctly rounded.
 *   coeffs (rows x num_coeffs): l[i] = logf(e[i] + 1e-12f) with the libm crate's logf (as the cepstrum), then out[j] = sum_i l[i] *
 *     C[i][j], i ascending from a +0 seed, one multiply and one add per term, C the table of kofft_hip_dct_direct_f32(ctx, 2, ..) at
 *     n = num_mel (dct::dct2, dct.rs:134-146), j < num_coeffs.
 * NaNs come out in the reference's places.  Checks, in this order and before the context or the device is touched: rows == 0 ->
 * KOFFT_OK; (mfcc) num_coeffs > num_mel -> INVALID_VALUE (cepstrum.rs:79); bins null -> KOFFT_ERR_NULL; bins not nondecreasing ->
 * INVALID_VALUE (the reference underflows a usize); n_fft > 2^24 or num_mel > 4096 (the bound of the direct table) ->
 * KOFFT_ERR_UNSUPPORTED; a null data pointer or context -> KOFFT_ERR_NULL; (device pointers) input and output overlap ->
 * INVALID_VALUE.  num_mel == 0 and num_coeffs == 0 are KOFFT_OK with nothing written; n_fft == 0 gives +0 energies and the MFCCs of
 * logf(1e-12f) rows, as the reference.  The kofft_hip_dev_* forms are asynchronous on the context's stream (named so for the reason
 * given at the chirp-Z entries; their guard-band cases live in tests/test_gpu_mfcc_footprint.py).  A context keeps the plans of its
 * four most recently used (bins, n_fft, num_mel) on the device until kofft_hip_release_scratch or kofft_hip_destroy.
 * Routes of the MFCC, the same bytes.  The fused kernel (a lane owns a row from its magnitudes to its coefficients; energies never
 * reach memory) fits num_mel <= 128: 256 bytes of LDS per filter and workgroup next to the 8.25 KiB staging tile, 40.25 KiB at 128,
 * three workgroups per CU.  The composed route runs through the context's scratch: filterbank kernel, pointwise log, the direct
 * DCT-II kernels on rows of num_mel, a copy of the first num_coeffs columns.  kofft_hip_set_mfcc_fused(ctx, mode): 1, the default,
 * takes the fused kernel where it measured faster (num_mel <= 80 and num_coeffs <= 16: DESIGN 5.21) and the composed route
 * elsewhere; 0 every call composed; 2 the fused kernel wherever it fits (A/B measurements and tests); anything else ->
 * INVALID_VALUE. */
int kofft_hip_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *mags, float *energies, size_t n_fft, size_t rows, const uint64_t *bins,
                                 size_t num_mel);
int kofft_hip_dev_mel_filterbank_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_energies, size_t n_fft, size_t rows,
                                     const uint64_t *bins, size_t num_mel);
int kofft_hip_mfcc_f32(kofft_hip_ctx *ctx, const float *mags, float *coeffs, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
                       size_t num_coeffs);
int kofft_hip_dev_mfcc_f32(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const uint64_t *bins,
                           size_t num_mel, size_t num_coeffs);
int kofft_hip_set_mfcc_fused(kofft_hip_ctx *ctx, int on);
/* Host only: the edges of cepstrum.rs:38-50, bins = num_filters + 2 values: mel_max = 2595 * log10f(1 + (rate / 2) / 700), point i =
 * 700 * (powf(10, ((mel_max * i) / (num_filters + 1)) / 2595) - 1), bins[i] = floorf(point * (n_fft + 1) / rate) as usize, all f32 in
 * Rust's parse order, the cast saturating (NaN and negatives give 0).  log10f and powf are GLIBC's, where the reference calls the
 * libm crate's: the result equals the crate's edges wherever the exact edge is not within an ulp of an integer.  The known case
 * that is not pinned: with an odd n_fft the last edge is the integer (n_fft + 1) / 2 in exact arithmetic and hangs on the last bit
 * of both functions.  A Rust caller should take the edges from the shim (kofft-hip: mel_bins), which computes them with the crate
 * itself.  num_filters > 4096 -> KOFFT_ERR_UNSUPPORTED; bins null -> KOFFT_ERR_NULL. */
int kofft_hip_mel_bins_f32(float sample_rate, size_t n_fft, size_t num_filters, uint64_t *bins);

/* ---- audio front end: rows of signals -> mel energies / MFCCs in one call ----------------------
 * stft_magnitudes -> mel_filterbank (-> logf -> dct2) over `rows` signals of `len` samples, row r at signal + r * row_stride, `frames`
 * frames per row, without the rows * frames * (win_len / 2) magnitudes ever being the caller's to hold.  energies is rows * frames *
 * num_mel floats, coeffs rows * frames * num_coeffs, both dense and frame-major within a row.  bins is a HOST pointer in both forms,
 * num_mel + 2 nondecreasing values, read before the call returns, exactly as in kofft_hip_mfcc_f32; n_fft of the mel stage is
 * win_len / 2, the length of a stft_magnitudes row.
 * Contract.  Let M be the magnitudes of frame f of row r.  window == NULL: M is what kofft_hip_stft_magnitudes_rows_f32 writes for
 * that frame (window::hann(win_len), bins 0 .. win_len/2 - 1, sqrt(re*re + im*im) un-fused, the root correctly rounded).  A window
 * given (win_len values; a device pointer in the kofft_hip_dev_* forms): the same expression over kofft_hip_stft_rows_f32's frames
 * for that window, bins < win_len/2.  A frame past the end of its row reads +0, never the head of row r + 1.  The output row is then
 * exactly what kofft_hip_mel_filterbank_f32 / kofft_hip_mfcc_f32 return for M with the same bins: the reference's summation order per
 * filter, logf(e + 1e-12f) with the libm crate's logf, the truncated dct::dct2 over the direct table of num_mel ascending from +0, one
 * multiply and one add per term, nothing fused; NaNs land where the two calls put them.  No maximum is computed.
 * Checks, in this order and before the context or the device is touched -- the STFT rows' first, then the mel ones:
 *   hop == 0 -> INVALID_HOP_SIZE; frames < ceil(len / hop) -> MISMATCHED_LENGTHS; rows == 0 or frames == 0 -> KOFFT_OK, nothing
 *   touched; win_len == 0 -> EMPTY_INPUT; win_len beyond the complex limits (kofft_hip_stft_rows_f32's) -> UNSUPPORTED; rows > 1 and
 *   row_stride < len -> INVALID_VALUE; (mfcc) num_coeffs > num_mel -> INVALID_VALUE; bins null -> KOFFT_ERR_NULL; bins decreasing ->
 *   INVALID_VALUE; num_mel > 4096 (or win_len / 2 > 2^24, the mel stage's bound) -> UNSUPPORTED; a null data pointer (signal with
 *   len > 0, the output) or a null context -> KOFFT_ERR_NULL; (device forms) the output overlapping the signal or the window ->
 *   INVALID_VALUE; num_mel == 0 or (mfcc) num_coeffs == 0 -> KOFFT_OK with nothing written.
 * win_len == 1 gives n_fft == 0: +0 energies and the MFCCs of logf(1e-12f) rows, as kofft_hip_mfcc_f32 at n_fft == 0.
 * Routes, the same bytes.  The fused kernel (power-of-two win_len 64 .. 2048, num_mel <= 128) keeps a frame's magnitudes, its log-mel
 * values and the DCT in LDS; the magnitudes never reach memory.  The composed route writes whole frames of magnitudes into the
 * context's scratch (KOFFT_HIP_SCRATCH_CHUNK_MB at a time, no maximum) and runs the mel / MFCC device path on them: every other
 * window length (Bluestein lengths such as 400 too) and more filters.  kofft_hip_set_frontend_fused(ctx, mode): 1, the default, the
 * measured choice (the composed route at every shape, which measured faster than the fused kernel and never slower than the
 * two calls); 0 every call composed; 2 the fused kernel wherever it fits (A/B measurements and tests); anything
 * else -> INVALID_VALUE.  The kofft_hip_dev_* forms are asynchronous on the context's stream (named so for the reason given at the
 * chirp-Z entries; their guard-band cases live in tests/test_gpu_frontend_footprint.py). */
int kofft_hip_stft_mel_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                                size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, float *energies);
int kofft_hip_dev_stft_mel_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                    const float *d_window, size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel,
                                    float *d_energies);
int kofft_hip_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                                 size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel, size_t num_coeffs,
                                 float *coeffs);
int kofft_hip_dev_stft_mfcc_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                     const float *d_window, size_t win_len, size_t hop, size_t frames, const uint64_t *bins, size_t num_mel,
                                     size_t num_coeffs, float *d_coeffs);
int kofft_hip_set_frontend_fused(kofft_hip_ctx *ctx, int mode);

/* ---- spectrogram colour helpers: magnitudes -> dB -> RGB picture -----------------------------
 * visual::spectrogram's magnitude_to_db, db_scale, map_color_u8 / _u16, color_from_magnitude_*, map_bin_to_pixel and log_scale_bins
 * (visual/spectrogram.rs:96-234), f32 only like the reference, on the magnitudes kofft_hip_dev_stft_magnitudes_rows_f32 leaves on the
 * device.  max_mag is a POINTER to one float: a host pointer in the host forms, a device pointer in the kofft_hip_dev_* forms (the
 * d_max of the magnitudes call: no host synchronisation in between).
 * The arithmetic contract.  log10 is the LIBM CRATE's log10f (the musl / FreeBSD e_log10f.c port, restated in
 * kofft_amd/csrc/libm_log10f.hip.h), which is what a build of the reference without a platform libm computes; with `std` the reference
 * calls the platform's log10f, and its own bytes differ from platform to platform.  Everything else is the reference's f32 operation
 * order, one rounding per operation, nothing fused: the correctly rounded divisions `mag / max_mag`, by `dynamic_range`, by `-floor_db`
 * and by a palette segment's width, `20.0 *`, f32::max (a NaN loses; of two equal values the floor is returned), f32::clamp (a NaN
 * stays), the palettes, f32::round for Gray, and `as u8` as a truncating, saturating cast with NaN -> 0.
 *   magnitude_to_db: max_mag <= 0 or mag <= 0 -> floor_db; else max(20 * log10f(mag / max_mag), floor_db).
 *   db_scale: clamp((20 * log10f(max(mag / max_mag, 1e-10)) + dynamic_range) / dynamic_range, 0, 1).
 *   render: mags[frames][bins] -> pixels.  mode 0: map_color_u8((magnitude_to_db(mag, max_mag, level) - level) / -level), `level` the
 *     floor in dB (color_from_magnitude_u8); mode 1: map_color_u8(db_scale(mag, max_mag, level)), `level` the dynamic range.  cmap:
 *     KOFFT_CMAP_*, the reference's declaration order; Fire, Legacy, Gray and Rainbow are implemented, VIRIDIS / PLASMA / INFERNO (the
 *     colorous crate's) return INVALID_VALUE.  depth 8: 3 bytes per pixel; depth 16: three native uint16_t, each the 8-bit value * 257
 *     (map_color_u16); the output needs no alignment.  scale 0: a pixel per bin; scale 1: every frame goes through
 *     log_scale_bins(frame, bins - 1) first -- pixel p is the sum of the bins b with pix_of_bin[b] == p in increasing order from +0,
 *     divided once by their count as f32, +0 without bins.  pix_of_bin (bins values, a HOST pointer in both forms, read before the
 *     call returns; NULL unless scale == 1) is an INPUT: kofft_hip_log_bin_map gives the reference-shaped one with glibc's logf, a
 *     caller with the libm crate can supply its own.  It must be nondecreasing (map_bin_to_pixel is, for every bins from 2 to 8192).
 *     layout 0: out[frames][bins][3]; layout 1: the picture out[bins][frames][3], row-major, bin b of frame x at row bins - 1 - b,
 *     column x (what the reference's programs build with put_pixel(x, height - 1 - y)).
 * Checks, in this order and before the context or the device is touched: count / frames / bins == 0 -> EMPTY_INPUT; an unknown mode,
 * cmap, depth, scale or layout, or a colorous palette -> INVALID_VALUE; scale == 1 with a null table, a table entry >= bins or a table
 * that decreases -> INVALID_VALUE; bins > 2^24 or more than 2^31 - 1 tiles of 64 x 64 -> KOFFT_ERR_UNSUPPORTED; a null pointer or
 * context -> KOFFT_ERR_NULL; (device pointers) the output overlapping the input or max_mag -> INVALID_VALUE.  level and max_mag are not
 * validated: the reference validates neither.  The kofft_hip_dev_* forms are asynchronous on the context's stream.  A context keeps
 * the pixel ranges of its four most recently used tables on the device until kofft_hip_release_scratch or kofft_hip_destroy.
 * kofft_hip_set_spectrogram_transpose(ctx, on): 1, the default, writes layout 1 through an LDS tile (whole dwords per picture row);
 * 0 lets every lane store its own bytes; the same bytes (which measured faster). */
#define KOFFT_CMAP_FIRE 0
#define KOFFT_CMAP_LEGACY 1
#define KOFFT_CMAP_GRAY 2
#define KOFFT_CMAP_VIRIDIS 3
#define KOFFT_CMAP_PLASMA 4
#define KOFFT_CMAP_INFERNO 5
#define KOFFT_CMAP_RAINBOW 6
int kofft_hip_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float floor_db, float *out);
int kofft_hip_dev_magnitude_to_db_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float floor_db,
                                      float *d_out);
int kofft_hip_db_scale_f32(kofft_hip_ctx *ctx, const float *mags, size_t count, const float *max_mag, float dynamic_range, float *out);
int kofft_hip_dev_db_scale_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t count, const float *d_max_mag, float dynamic_range,
                               float *d_out);
int kofft_hip_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *mags, size_t frames, size_t bins, const float *max_mag, int mode,
                                     float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin, void *out);
int kofft_hip_dev_spectrogram_render_f32(kofft_hip_ctx *ctx, const float *d_mags, size_t frames, size_t bins, const float *d_max_mag,
                                         int mode, float level, int cmap, int depth, int scale, int layout, const uint32_t *pix_of_bin,
                                         void *d_out);
int kofft_hip_set_spectrogram_transpose(kofft_hip_ctx *ctx, int on);
/* ---- rows of audio -> spectrogram pictures in one call --------------------------
 * What examples/spectrogram.rs and sanity-check do (stft_magnitudes, its maximum, a colour per bin) and what web-spectrogram's
 * State::compute_frame does a frame at a time with a running maximum, for `rows` signals at once: the magnitudes never belong to
 * the caller (they pass through the context's scratch, at most KOFFT_HIP_SCRATCH_CHUNK_MB of it at a time).
 * Let M[r][f][o], o < win_len/2, be the magnitudes kofft_hip_stft_mel_f32 defines for the same signal, window (NULL: hann(win_len)),
 * win_len, hop and frames (+0 past the end of a row, never the head of row r + 1).  Picture r is, byte for byte, what
 * kofft_hip_spectrogram_render_f32 writes for M[r] with the same mode, level, cmap, depth, scale, layout and pix_of_bin (a HOST
 * pointer in both forms) and the maximum that max_mode chooses; pictures are dense, picture r at out + r * frames * (win_len/2) *
 * bytes_per_pixel.  channels 3: RGB as in the render; channels 4 (depth 8 only): R, G, B, 255 -- in layout 0 compute_frame's rows.
 * The output needs no alignment.
 *   max_mode 0, the row's maximum: stft_magnitudes' (`if mag > max` from +0: a NaN is never selected); max_out[r] is
 *     kofft_hip_stft_magnitudes_rows_f32's max_mag[r] bit for bit (there: Hann, frames == ceil(len / hop)).
 *   max_mode 1, the running maximum: compute_frame's.  Per row m starts at 1e-12f; walking frames, then bins, in ascending order,
 *     `if mag > m { m = mag }` runs BEFORE the pixel is coloured with m (an inclusive prefix); max_out[r] is the final m.  scale == 1
 *     is refused: the reference defines no position for the maximum under log_scale_bins.
 *   max_mode 2, given: max_in[r] is used unvalidated, as in the render; max_out, if given, receives a copy; nothing is computed.
 * max_out may be NULL in every mode; max_in is read in mode 2 only.  In the kofft_hip_dev_* forms signal, window, max_in, max_out
 * and out are device pointers, the call is asynchronous on the context's stream and nothing synchronises with the host.
 * Checks, in this order and before the context or the device is touched:
 *   1. kofft_hip_stft_mel_f32's STFT checks: hop == 0 -> INVALID_HOP_SIZE; frames < ceil(len / hop) -> MISMATCHED_LENGTHS; rows == 0
 *      or frames == 0 -> KOFFT_OK, nothing written; win_len == 0 -> EMPTY_INPUT; its limits -> KOFFT_ERR_UNSUPPORTED; rows > 1 with
 *      row_stride < len -> INVALID_VALUE;
 *   2. the render's: an unknown mode, cmap, depth, scale or layout, a colorous palette, scale == 1 with a null table, an entry
 *      >= win_len/2 or a table that decreases -> INVALID_VALUE;
 *   3. an unknown max_mode, channels not 3 or 4, channels == 4 with depth 16, max_mode == 1 with scale == 1 -> INVALID_VALUE;
 *      win_len/2 > 2^24 -> KOFFT_ERR_UNSUPPORTED;
 *   4. win_len == 1 (no bins) -> KOFFT_OK with nothing written but max_out: +0 (mode 0), 1e-12f (mode 1), max_in's copy (mode 2; a
 *      null max_in is KOFFT_ERR_NULL; the device form needs the context to write and returns KOFFT_ERR_NULL without one);
 *   5. a null context, out, signal (len > 0) or (mode 2) max_in -> KOFFT_ERR_NULL;
 *   6. (device forms) out overlapping the signal, the window, max_in or max_out -> INVALID_VALUE. */
int kofft_hip_stft_picture_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride, const float *window,
                               size_t win_len, size_t hop, size_t frames, int max_mode, const float *max_in, float *max_out, int mode,
                               float level, int cmap, int depth, int channels, int scale, int layout, const uint32_t *pix_of_bin, void *out);
int kofft_hip_dev_stft_picture_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride,
                                   const float *d_window, size_t win_len, size_t hop, size_t frames, int max_mode, const float *d_max_in,
                                   float *d_max_out, int mode, float level, int cmap, int depth, int channels, int scale, int layout,
                                   const uint32_t *pix_of_bin, void *d_out);
/* Host only: pix_of_bin[b] = map_bin_to_pixel(b, bins - 1) (spectrogram.rs:209-217) for every b < bins: max_bin == 0 -> 0, else
 * floor(max_bin as f32 * ln(b as f32 + 1) / ln(max_bin as f32 + 1)) as a saturating cast, f32 in Rust's parse order with GLIBC's logf.
 * bins == 0 -> EMPTY_INPUT; bins > 2^24 -> KOFFT_ERR_UNSUPPORTED; a null pointer -> KOFFT_ERR_NULL. */
int kofft_hip_log_bin_map(size_t bins, uint32_t *pix_of_bin);
/* Host only: map_color_u8(t, cmap) (spectrogram.rs:113-160) for a legend.  A colorous palette or an unknown cmap -> INVALID_VALUE;
 * rgb null -> KOFFT_ERR_NULL. */
int kofft_hip_map_color_u8(float t, int cmap, unsigned char *rgb);

/* ---- direct DCT-I..IV and DST-I..IV ---------------------------------------------
 * dct::dct1 .. dct4 (dct.rs:108-176) and dst::dst1 .. dst4 (dst.rs:89-146), f32 only like
 * the reference (there is no f64 direct transform), on `batch` contiguous rows of n reals;
 * out: batch * n reals.  These are the naive O(n^2) sums: kofft_hip_dct_direct_f32(ctx, 2,
 * ..) is dct::dct2, NOT DctPlanner::plan_dct2 (kofft_hip_dct2_f32, FFT-based), and the two do
 * not return the same bytes.  Per output k: sum = init, then sum += x'[i] * C[i][k] for
 * every i of the kind's range in increasing order, one f32 multiply and one f32 add per term
 * (never fused), C[i][k] = glibc cosf / sinf of the reference's f32 angle:
 *   DCT-I   init x0 + x[n-1] (k even) / x0 + (-x[n-1]) (k odd), [2 * x0] at n == 1; i = 1 ..
 *           n-2; x' = 2 * x; angle (PI / (n - 1) * i) * k                   (dct.rs:108-131)
 *   DCT-II  init +0; i = 0 .. n-1; angle (PI / n * (i + 0.5)) * k           (dct.rs:134-146)
 *   DCT-III init x0 / 2; i = 1 .. n-1; angle (PI / n * i) * (k + 0.5)       (dct.rs:149-161)
 *   DCT-IV  init +0; i = 0 .. n-1; angle (PI / n * (i + 0.5)) * (k + 0.5)   (dct.rs:164-176)
 *   DST-I   init +0; i = 0 .. n-1; angle ((i + 1) * (k + 1)) * (PI / (n + 1)) (dst.rs:89-101)
 *   DST-II  init +0; i = 0 .. n-1; angle (PI / n * (i + 0.5)) * (k + 1)     (dst.rs:104-116)
 *   DST-III init x0 / 2; i = 1 .. n-1; angle (PI / n * (k + 0.5)) * i       (dst.rs:119-131)
 *   DST-IV  init +0; i = 0 .. n-1; angle (PI / n * (i + 0.5)) * (k + 0.5)   (dst.rs:134-146)
 * Checks, in this order and before the context or the device is touched: type not 1 .. 4 ->
 * INVALID_VALUE; batch == 0 -> KOFFT_OK; n == 0 -> KOFFT_OK (an empty result, as the
 * reference), but EMPTY_INPUT for type 3 (dct3 / dst3 index input[0] unchecked: the reference
 * panics); n > 4096 -> KOFFT_ERR_UNSUPPORTED (the bound of the n x n table, 64 MiB at 4096);
 * a null pointer or context -> KOFFT_ERR_NULL.  The host form allows in == out (the
 * reference's batch_* work in place).  _dev: device pointers, asynchronous on the context's
 * stream; in and out must not overlap (the tiles of one row run in different workgroups): an
 * overlap returns INVALID_VALUE.  The first call of a (context, kind, n) builds the table on
 * the host (up to 16 threads; about 64 MiB of cosf / sinf at n = 4096) and keeps it on the
 * device until the context is destroyed.  kofft_hip_set_direct_tiled(ctx, 0) sends every call
 * of that context to the simple kernel (one lane per output) instead of the tiled one: the
 * same bytes (A/B measurements and tests). */
int kofft_hip_dct_direct_f32(kofft_hip_ctx *ctx, int type, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_dct_direct_f32_dev(kofft_hip_ctx *ctx, int type, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_dst_direct_f32(kofft_hip_ctx *ctx, int type, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_dst_direct_f32_dev(kofft_hip_ctx *ctx, int type, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_set_direct_tiled(kofft_hip_ctx *ctx, int on);
/* The 4096-point c32 streaming kernel walks the first rows of a batch with the stride of its grid and
 * hands out the last ones by claim (one fetch-add per row), so that a workgroup that falls behind
 * leaves rows to the others.  pct = 0 .. 100: the share of the batch that is claimed (100: all of
 * it; 0: only what the grid's stride leaves over); pct < 0: the library's measured default;
 * pct > 100 -> INVALID_VALUE.  The same bytes at every setting (A/B measurements and tests). */
int kofft_hip_set_persist_claim_pct(kofft_hip_ctx *ctx, int pct);
/* Tests only: waits for the context's stream, then reads back the first word of each of the nine
 * 128-byte lines of the claim hand-out (the claim words, one per piece of the claimed rows, in the
 * first lines; the arrival word in the last), which every launch leaves at zero.  ctx or out null ->
 * KOFFT_ERR_NULL. */
int kofft_hip_persist_claim_debug(kofft_hip_ctx *ctx, unsigned out[9]);
/* Which way that kernel walks a batch.  Rows are independent, so every setting computes the same
 * bytes; only the order in which rows are taken and the cache policy of some stores differ.
 *   mode -1 (default): a call whose input range or output range is exactly the range the context's
 *           previous call of this kernel wrote walks the batch from the other end than that call
 *           did (the rows written last are read first); any other call walks ascending.  Other
 *           calls through the context do not clear what is remembered: a stale record costs at
 *           most one needless change of direction.  A captured graph replays the directions it
 *           was captured with.
 *   mode 0: always ascending, no kept zone: the kernel as it was before this knob existed.
 *   mode 1 / 2: always ascending / descending, with the kept zone (A/B measurements and tests).
 * The kept zone is the end of a walk, `bytes` long, stored with the default cache policy instead of
 * the streaming one; 0 switches it off, and under mode -1 it is off for batches smaller than twice
 * the zone (modes 1 and 2 clamp it to the batch).  mode outside -1 .. 2 -> INVALID_VALUE.
 * Calls, not environment variables, like kofft_hip_set_persist_claim_pct. */
int kofft_hip_set_persist_walk(kofft_hip_ctx *ctx, int mode);
int kofft_hip_set_persist_keep_bytes(kofft_hip_ctx *ctx, size_t bytes);
/* Tests only, host-side state, no synchronisation: out[0] = launches of that kernel through the
 * context so far; of the last one: out[1] = 1 if it walked descending, out[2] = the first walk index
 * of its kept zone (= its batch: none), out[3] = its batch.  ctx or out null -> KOFFT_ERR_NULL. */
int kofft_hip_persist_walk_debug(kofft_hip_ctx *ctx, unsigned long long out[4]);
/* The tables of the direct transforms, host only (tests): C = n * n floats, C[i * n + k] as
 * above; rows outside the kind's i range are +0.  type not 1 .. 4 -> INVALID_VALUE; n == 0 ->
 * KOFFT_OK; n > 4096 -> KOFFT_ERR_UNSUPPORTED; C null -> KOFFT_ERR_NULL. */
int kofft_hip_dct_direct_table_f32(int type, size_t n, float *C);
int kofft_hip_dst_direct_table_f32(int type, size_t n, float *C);
/* DstPlanner::plan_dst2 / 3 / 4 (dst.rs:41-77), host only: out[i] = sin(factor * (i + off)),
 * factor = pi / n, i < n, off = 0.5 (types 2, 4) or 0.0 (type 3).  f32: glibc sinf of f32
 * arithmetic; f64: glibc sin, with i and n converted through f32 as T::from_f32(i as f32)
 * does.  type not 2 .. 4 -> INVALID_VALUE; n == 0 -> KOFFT_OK; out null -> KOFFT_ERR_NULL. */
int kofft_hip_dst_planner_table_f32(int type, size_t n, float *out);
int kofft_hip_dst_planner_table_f64(int type, size_t n, double *out);

/* ---- chirp-Z transform and Goertzel detector -----------------------------------------
 * czt::czt_f32 (czt.rs:16-54) and goertzel::goertzel_f32 (goertzel.rs:16-36, the std form), f32 only like the reference, on
 * `batch` contiguous rows of n reals; every operation is one f32 rounding in the reference's order, never fused.
 *
 * czt: out = batch * m complex (re, im interleaved).  Per bin k: out = (+0, +0), wnk = apow = (1, 0), then for i ascending
 *   t = apow * wnk;  out.re += x[i] * t.re;  out.im += x[i] * t.im;  wnk = wnk * w^k;  apow = apow * a_inv
 * with the un-fused complex product (p.r * q.r - p.i * q.i, p.r * q.i + p.i * q.r), w^k = w multiplied k times into (1, 0) and
 * a_inv = (ar / denom, -ai / denom), denom = ar * ar + ai * ai, (0, 0) when denom == 0.  Checks, in this order, before any device
 * call: batch == 0 or m == 0 -> KOFFT_OK, nothing written; n > 4096 or m > 4096 -> KOFFT_ERR_UNSUPPORTED; a null context or pointer ->
 * KOFFT_ERR_NULL; (device pointers) in and out overlap -> INVALID_VALUE.  n == 0 writes m bins of (+0, +0) per row, as the reference
 * does.  Routes, all giving the same bytes (kofft_hip_set_czt_route): 1 sums on the fly, one lane per (row, bin); 2 builds the
 * n x 2m table C[i][k] = apow[i] * (w^k)^i on the device and runs the sums on the kernels of the direct DCT / DST; 0, the default,
 * chooses by batch and by whether the table is already there; anything else -> INVALID_VALUE.  A context keeps the
 * tables of its four most recently used (n, m, w, a) -- up to 128 MiB each at n = m = 4096 -- until kofft_hip_release_scratch or
 * kofft_hip_destroy.
 *
 * goertzel: nfreq target frequencies per call, out = batch * nfreq reals, out[b * nfreq + j] the reference's result for row b and
 * target_freqs[j]; nfreq == 1 is the reference's call.  Per frequency, on the host: k = floorf((f * n) / rate), omega =
 * ((2 * PI) * k) / n, coeff = 2 * cosf(omega) (n as f32, glibc cosf).  Per row: s = (x + coeff * s_prev) - s_prev2 from +0 seeds, then
 * sqrtf((s_prev2 * s_prev2 + s_prev * s_prev) - (coeff * s_prev) * s_prev2), correctly rounded; a negative or NaN power gives NaN.
 * Checks, in this order: batch == 0 -> KOFFT_OK; n == 0 -> EMPTY_INPUT; sample_rate <= 0 -> INVALID_VALUE (a NaN rate passes, as in
 * the reference); nfreq == 0 -> KOFFT_OK; n > 2^26 or nfreq > 1024 -> KOFFT_ERR_UNSUPPORTED; a null context or pointer ->
 * KOFFT_ERR_NULL; (device pointers) in and out overlap -> INVALID_VALUE.  target_freqs is a HOST pointer in both forms; the
 * device-pointer form reads it before it returns and brings the coefficients over in kernel arguments, so it stays asynchronous.
 *
 * The device-pointer forms are named kofft_hip_dev_*, not *_dev: the guard-band table of tests/test_gpu_footprint.py is matched
 * against every *_dev name of this header and predates these calls; their guard-band cases live in tests/test_gpu_spectral.py. */
int kofft_hip_czt_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t m, float wr, float wi, float ar, float ai,
                      size_t batch);
int kofft_hip_dev_czt_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t m, float wr, float wi, float ar, float ai,
                          size_t batch);
int kofft_hip_goertzel_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch, float sample_rate,
                           const float *target_freqs, size_t nfreq);
int kofft_hip_dev_goertzel_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch, float sample_rate,
                               const float *target_freqs, size_t nfreq);
int kofft_hip_set_czt_route(kofft_hip_ctx *ctx, int mode);
/* Host only (tests): the chirp-Z table computed on the host with the same recurrences, C = n * 2m floats, C[i * 2m + 2k], [.. + 1] =
 * apow[i] * (w^k)^i.  n == 0 or m == 0 -> KOFFT_OK; n or m > 4096 -> KOFFT_ERR_UNSUPPORTED; C null -> KOFFT_ERR_NULL. */
int kofft_hip_czt_table_f32(size_t n, size_t m, float wr, float wi, float ar, float ai, float *C);
/* Host only: coeff[j] as above.  n == 0 -> EMPTY_INPUT; sample_rate <= 0 -> INVALID_VALUE; nfreq == 0 -> KOFFT_OK; n > 2^26 or
 * nfreq > 1024 -> KOFFT_ERR_UNSUPPORTED; a null pointer -> KOFFT_ERR_NULL. */
int kofft_hip_goertzel_coeff_f32(size_t n, float sample_rate, const float *target_freqs, size_t nfreq, float *coeff);

/* ---- Hartley transform ------------------------------------------------------------------
 * hartley::dht / batch / multi_channel (hartley.rs:12-57), f32 only like the reference, on `batch` contiguous rows of n reals in and
 * out:  out[b][k] = sum_i x[b][i] * H[i][k], the sum seeded with +0, i ascending, one f32 multiply and one f32 add per term, never
 * fused.  H[i][k] = cosf(a) + sinf(a) (one f32 add), a = factor * ((i * k) as f32), factor = (2.0 * PI) / (n as f32), where cosf and
 * sinf are the libm crate's (hartley.rs:8), not glibc's: kofft_amd/csrc/libm_trigf.hip.h restates them.  H is symmetric and depends
 * on n only; a context keeps the n x n table of every length it has seen (64 MiB at n = 4096) until kofft_hip_destroy.
 * Checks, in this order and before the context or the device is touched: batch == 0 -> KOFFT_OK; n == 0 -> KOFFT_OK (an empty
 * result, as the reference); n > 4096 -> KOFFT_ERR_UNSUPPORTED (the bound of the table); a null pointer or context -> KOFFT_ERR_NULL;
 * (device pointers) in and out overlap -> INVALID_VALUE.  The host form allows in == out (hartley::batch works in place).
 * kofft_hip_dev_dht_f32: device pointers, asynchronous on the context's stream -- the first call of a length included: the table is
 * built by a kernel on that stream.  (Named kofft_hip_dev_* for the reason given at the chirp-Z entries; its guard-band cases live
 * in tests/test_gpu_hartley.py.)  The sums run on the kernels of the direct DCT / DST by the same rule (kofft_hip_set_direct_tiled
 * applies).  kofft_hip_set_dht_table_device(ctx, 0): tables of lengths not seen yet are built on the host (up to 16 threads) and
 * uploaded instead -- the same bytes (A/B measurements and tests); on: the default. */
int kofft_hip_dht_f32(kofft_hip_ctx *ctx, const float *in, float *out, size_t n, size_t batch);
int kofft_hip_dev_dht_f32(kofft_hip_ctx *ctx, const float *d_in, float *d_out, size_t n, size_t batch);
int kofft_hip_set_dht_table_device(kofft_hip_ctx *ctx, int on);
/* Host only (tests): H = n * n floats, H[i * n + k] as above.  n == 0 -> KOFFT_OK; n > 4096 -> KOFFT_ERR_UNSUPPORTED; H null ->
 * KOFFT_ERR_NULL. */
int kofft_hip_dht_table_f32(size_t n, float *H);
/* Host only (tests): the restated cosf / sinf of `count` arguments.  count == 0 -> KOFFT_OK; a null pointer -> KOFFT_ERR_NULL; any
 * finite |x| >= 0x4dc90fdb (about 4.2e8; the crate's rem_pio2_large is not restated) -> KOFFT_ERR_UNSUPPORTED, nothing written. */
int kofft_hip_libm_trigf(const float *x, size_t count, float *cos_out, float *sin_out);

/* ---- windows beyond Hann, host only like kofft_hip_hann_f32 -----------------------------------
 * window::hamming / blackman / kaiser (window.rs:31-61) and window_more::tukey / bartlett / bohman / nuttall (window_more.rs:13-64):
 * out = len floats, every expression in f32 in Rust's parse order (`2.0 * PI * i as f32 / len as f32` is ((2 PI) * i) / len).
 * `.cos()` is glibc's cosf (hamming, blackman, tukey); cosf / sinf imported from the libm crate are the restated ones (bohman,
 * nuttall).  param: kaiser's beta, tukey's alpha, ignored by the rest.  Checks, in this order: kind not one of the constants ->
 * INVALID_VALUE; len == 0 -> KOFFT_OK, but EMPTY_INPUT for kaiser (the reference computes `len - 1` in usize: it underflows); out
 * null -> KOFFT_ERR_NULL.  Edge cases, as the reference:
 *   len == 1  hamming 0.08 (0.54 - 0.46), blackman 0.42 - 0.5 + 0.08, tukey 1.0; bartlett, bohman, nuttall and kaiser divide zero by zero: NaN.
 *   kaiser    bessel0 is the 19-term series as written; sqrtf the correctly rounded root.
 *   tukey     alpha is clamped to [0, 1] by f32::clamp, which keeps a NaN; edge = floorf(alpha * (len - 1) / 2) `as usize`, a
 *             saturating cast (NaN and negatives give 0): alpha <= 0 and a NaN alpha give len ones. */
#define KOFFT_WINDOW_HAMMING 0
#define KOFFT_WINDOW_BLACKMAN 1
#define KOFFT_WINDOW_KAISER 2
#define KOFFT_WINDOW_TUKEY 3
#define KOFFT_WINDOW_BARTLETT 4
#define KOFFT_WINDOW_BOHMAN 5
#define KOFFT_WINDOW_NUTTALL 6
int kofft_hip_window_f32(int kind, size_t len, float param, float *out);

/* ---- wavelets -------------------------------------------------------------------
 * wavelet::* (wavelet.rs:12-117, 154-567), f32 only like the reference.  The wavelet ids: */
#define KOFFT_WAVELET_HAAR 0
#define KOFFT_WAVELET_DB2 1
#define KOFFT_WAVELET_DB4 2
#define KOFFT_WAVELET_SYM4 3
#define KOFFT_WAVELET_COIF1 4
/* One level, `batch` contiguous rows.  dwt: rows of len samples in; approx and detail: batch rows of len / 2 each (an odd len
 * contributes len / 2 outputs, its reflection runs over the whole odd length; len == 1 writes nothing), as <name>_forward.  idwt:
 * rows of n approximations and n details in; out: batch rows of 2n, as <name>_inverse.
 * Multi level: multi_level_forward / multi_level_inverse with <name>_forward / <name>_inverse (the <name>_forward_multi /
 * _inverse_multi of the reference).  dwt_multi: approx holds batch rows of a_L; details holds the levels' details finest first, each
 * level packed [batch][a_l], one level after another, where a_0 = len and a_l = ceil(a_{l-1} / 2) (an odd row is padded with its last
 * sample before each level; kofft_hip_dwt_multi_lengths gives them).  levels == 0 copies the input to approx (no details; details
 * may be null).  idwt_multi: approx holds batch rows of n, details the levels' details packed as above, detail_lens[l] (finest
 * first) long; out: batch rows of n << levels.  Only the first n << (levels - 1 - l) entries of level l's detail rows are read.
 * The arithmetic is the reference's, term for term, never fused.
 * Checks, in this order and before the context or the device is touched: a wavelet id outside 0 .. 4 -> INVALID_VALUE; batch == 0
 * or len / n == 0 -> KOFFT_OK (an empty result, as the reference); idwt_multi: detail_lens null with levels > 0 -> KOFFT_ERR_NULL,
 * levels > 64 -> KOFFT_ERR_UNSUPPORTED (both before detail_lens is read), then a detail shorter than the approximation it is folded
 * into -> MISMATCHED_LENGTHS (the reference indexes past its end and panics; with the forward's own lengths this happens exactly
 * when one of a_1 .. a_{L-1} is odd); an input or output row (or a detail length) over 2^26 floats, or levels > 64 ->
 * KOFFT_ERR_UNSUPPORTED; a null context or pointer -> KOFFT_ERR_NULL.  _dev: device
 * pointers, asynchronous on the context's stream; an input that overlaps an output, or two outputs that overlap -> INVALID_VALUE.
 * Routes, all giving the same bytes: the fused kernels keep every level of rows of up to 16384 samples (dwt_multi: the input;
 * idwt_multi: the output) in LDS; the per-level route runs the single-level kernels level by level through context scratch.
 * kofft_hip_set_wavelet_fused(ctx, on): 1 (the default) takes the fused kernels only where they measured faster (per
 * wavelet and direction, at least two levels); 0 sends every call level by level; 2 takes the fused kernels wherever the row fits
 * (A/B measurements, tests); anything else -> INVALID_VALUE. */
int kofft_hip_dwt_f32(kofft_hip_ctx *ctx, int wavelet, const float *in, float *approx, float *detail, size_t len, size_t batch);
int kofft_hip_dwt_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_in, float *d_approx, float *d_detail, size_t len, size_t batch);
int kofft_hip_idwt_f32(kofft_hip_ctx *ctx, int wavelet, const float *approx, const float *detail, float *out, size_t n, size_t batch);
int kofft_hip_idwt_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_approx, const float *d_detail, float *d_out, size_t n, size_t batch);
int kofft_hip_dwt_multi_f32(kofft_hip_ctx *ctx, int wavelet, const float *in, float *approx, float *details, size_t len, size_t batch,
                            size_t levels);
int kofft_hip_dwt_multi_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_in, float *d_approx, float *d_details, size_t len,
                                size_t batch, size_t levels);
int kofft_hip_idwt_multi_f32(kofft_hip_ctx *ctx, int wavelet, const float *approx, const float *details, const size_t *detail_lens,
                             float *out, size_t n, size_t batch, size_t levels);
int kofft_hip_idwt_multi_f32_dev(kofft_hip_ctx *ctx, int wavelet, const float *d_approx, const float *d_details, const size_t *detail_lens,
                                 float *d_out, size_t n, size_t batch, size_t levels);
int kofft_hip_set_wavelet_fused(kofft_hip_ctx *ctx, int on);
/* Host only: lens[0 .. levels] = len, a_1 .. a_L (levels > 64 -> UNSUPPORTED, lens null -> NULL). */
int kofft_hip_dwt_multi_lengths(size_t len, size_t levels, size_t *lens);
/* Host only (tests): the library's coefficients, 8 floats each, +0 past the filter length.  Forward: lo = h (approximation), hi = g
 * (detail); inverse: lo multiplies the approximation, hi the detail (db2: gk / hk).  Haar has no arrays: all +0.  A wavelet id
 * outside 0 .. 4 -> INVALID_VALUE; lo or hi null -> NULL. */
int kofft_hip_wavelet_taps_f32(int wavelet, int inverse, float *lo, float *hi);

/* ---- STFT ---------------------------------------------------------------------
 * stft::stft (stft.rs:76-105): out = frames * win_len complex, contiguous (the
 * reference's &mut [Vec<Complex32>] flattened).  hop == 0 -> INVALID_HOP_SIZE;
 * frames < ceil(len/hop) -> MISMATCHED_LENGTHS; every provided frame is computed,
 * zero-padded past the end of the signal; win_len == 0 with frames > 0 -> EMPTY_INPUT.
 * The _dev form computes frames [first_frame, first_frame+count) of the same STFT
 * into d_out[0 .. count*win_len) -- the unit one rank owns when frames are sharded
 * across GPUs; it performs stft::parallel's checks only (stft.rs:232-263: hop != 0).
 */
int kofft_hip_stft_f32(kofft_hip_ctx *ctx, const float *signal, size_t len, const float *window,
                       size_t win_len, size_t hop, float *out, size_t frames);
/* stft::parallel (stft.rs:232-263): identical frames, but the only check is hop != 0 --
 * it does not require frames >= ceil(len/hop). */
int kofft_hip_stft_parallel_f32(kofft_hip_ctx *ctx, const float *signal, size_t len,
                                const float *window, size_t win_len, size_t hop, float *out,
                                size_t frames);
/* stft::frame (stft.rs:355-372) and StftStream::next_frame (stft.rs:186-205): the one frame
 * that starts at sample `start` (zero-padded past the end); frame_out: win_len complex. */
int kofft_hip_stft_frame_f32(kofft_hip_ctx *ctx, const float *signal, size_t len,
                             const float *window, size_t win_len, size_t start, float *frame_out);
int kofft_hip_stft_f32_dev(kofft_hip_ctx *ctx, const float *d_signal, size_t len,
                           const float *d_window, size_t win_len, size_t hop, float *d_out,
                           size_t first_frame, size_t count);

/* ---- ISTFT (SURVEY 8f "next" row 1) --------------------------------------------
 * stft::istft (stft.rs:117-156): every frame is inverse-transformed IN PLACE (frames_data:
 * frames * win_len complex, contiguous), then overlap-added into `output` (accumulated:
 * the reference does not clear it) with window-square normalisation where the sum exceeds
 * 1e-8; `scratch` receives the window-square sums.  hop == 0 -> INVALID_HOP_SIZE;
 * scratch_len != out_len -> MISMATCHED_LENGTHS.  The per-sample sums run in frame order,
 * exactly as the reference's loop nest does (no atomics). */
int kofft_hip_istft_f32(kofft_hip_ctx *ctx, float *frames_data, size_t frames, const float *window,
                        size_t win_len, size_t hop, float *output, size_t out_len, float *scratch,
                        size_t scratch_len);
int kofft_hip_istft_f32_dev(kofft_hip_ctx *ctx, float *d_frames, size_t frames, const float *d_window,
                            size_t win_len, size_t hop, float *d_output, size_t out_len,
                            float *d_scratch, size_t scratch_len);
/* stft::inverse_parallel (stft.rs:289-343): the same sums, but the frames are not modified and samples
 * whose window-square sum is <= 1e-8 are set to 0.  Only hop == 0 is rejected. */
int kofft_hip_istft_parallel_f32(kofft_hip_ctx *ctx, const float *frames_data, size_t frames,
                                 const float *window, size_t win_len, size_t hop, float *output,
                                 size_t out_len);
/* stft::inverse_frame (stft.rs:384-399): ifft(frame) in place, then output[start+i] += frame[i].re *
 * window[i] for start+i < out_len; no normalisation. */
int kofft_hip_istft_frame_f32(kofft_hip_ctx *ctx, float *frame, const float *window, size_t win_len,
                              size_t start, float *output, size_t out_len);

/* ---- STFT magnitudes (SURVEY 8f "next" row 2) --------------------------------------
 * visual::spectrogram::stft_magnitudes (visual/spectrogram.rs:52-76): STFT with a Hann window of
 * win_len (window::hann), keeping bins 0 .. win_len/2-1 of every frame as f32 magnitudes
 * sqrt(re*re + im*im), plus the maximum magnitude (0.0 if there are none; NaN never selected).
 * mags: frames * (win_len/2) floats, frames >= ceil(len/hop) (the reference allocates exactly that
 * many).  hop == 0 -> INVALID_HOP_SIZE (the reference would panic dividing by it).  The magnitude
 * is fused into the transform's store: 4x fewer output bytes than stft + a second pass. */
int kofft_hip_stft_magnitudes_f32(kofft_hip_ctx *ctx, const float *samples, size_t len, size_t win_len,
                                  size_t hop, float *mags, size_t frames, float *max_mag);
int kofft_hip_stft_magnitudes_f32_dev(kofft_hip_ctx *ctx, const float *d_samples, size_t len,
                                      size_t win_len, size_t hop, float *d_mags, size_t frames,
                                      float *d_max);

/* ---- the three STFT families over ROWS of signals ----
 * `rows` signals of `len` samples, row r at signal + r * row_stride (row_stride >= len, in floats; ignored
 * when rows == 1), one window of win_len, one hop, `frames` frames per row; every output is dense.  Row r of
 * every output is, bit for bit, what the single-signal entry above returns for signal r alone; a frame that
 * runs past the end of its row reads exactly +0, never the head of row r + 1.  One launch chain serves all
 * rows.  Checks, in order: hop == 0 -> INVALID_HOP_SIZE; (host forms and magnitudes) frames < ceil(len/hop)
 * -> MISMATCHED_LENGTHS; rows == 0 or frames == 0 -> KOFFT_OK, nothing touched (magnitudes with rows > 0:
 * max_mag zeroed); win_len == 0 -> EMPTY_INPUT; win_len beyond the complex limits -> UNSUPPORTED;
 * rows > 1 and row_stride < len -> INVALID_VALUE; then the pointers.
 * out: rows * frames * win_len complex.  mags: rows * frames * (win_len/2) floats, max_mag: rows floats.
 * The device-pointer forms are named kofft_hip_dev_* like the chirp-Z and split-complex ones (DESIGN.md 5.18:
 * the suite's coverage check of the *_dev names is tied to a case table these calls cannot join; their own
 * check is tests/test_stft_rows_cpu.py). */
int kofft_hip_stft_rows_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride,
                            const float *window, size_t win_len, size_t hop, float *out, size_t frames);
int kofft_hip_dev_stft_rows_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len,
                                size_t row_stride, const float *d_window, size_t win_len, size_t hop,
                                float *d_out, size_t frames);
int kofft_hip_stft_magnitudes_rows_f32(kofft_hip_ctx *ctx, const float *samples, size_t rows, size_t len,
                                       size_t row_stride, size_t win_len, size_t hop, float *mags,
                                       size_t frames, float *max_mag);
int kofft_hip_dev_stft_magnitudes_rows_f32(kofft_hip_ctx *ctx, const float *d_samples, size_t rows, size_t len,
                                           size_t row_stride, size_t win_len, size_t hop, float *d_mags,
                                           size_t frames, float *d_max);
/* stft::istft (mode 1) / stft::inverse_parallel (mode 2) per row: frames_data rows * frames * win_len complex,
 * output rows * out_len (accumulated into), scratch rows * out_len (scratch_len == out_len, per row).  Checks
 * and side effects are the single-signal forms': istft transforms the frames in place and leaves the
 * window-square sums in scratch; the parallel form leaves the frames alone and writes 0 where the sum is
 * <= 1e-8.  The device parallel form inverse-transforms copies of the frames in scratch the context owns
 * (until kofft_hip_release_scratch / destroy): whole rows at a time, at most 512 MiB, or one row's frames
 * where a single row is larger. */
int kofft_hip_istft_rows_f32(kofft_hip_ctx *ctx, float *frames_data, size_t rows, size_t frames,
                             const float *window, size_t win_len, size_t hop, float *output, size_t out_len,
                             float *scratch, size_t scratch_len);
int kofft_hip_dev_istft_rows_f32(kofft_hip_ctx *ctx, float *d_frames, size_t rows, size_t frames,
                                 const float *d_window, size_t win_len, size_t hop, float *d_output,
                                 size_t out_len, float *d_scratch, size_t scratch_len);
int kofft_hip_istft_parallel_rows_f32(kofft_hip_ctx *ctx, const float *frames_data, size_t rows, size_t frames,
                                      const float *window, size_t win_len, size_t hop, float *output,
                                      size_t out_len);
int kofft_hip_dev_istft_parallel_rows_f32(kofft_hip_ctx *ctx, const float *d_frames, size_t rows, size_t frames,
                                          const float *d_window, size_t win_len, size_t hop, float *d_output,
                                          size_t out_len);

/* ---- one-sided STFT over rows of signals, and its inverse ----
 * K = win_len / 2 + 1 (integer division).  Forward: the arguments, checks and check order of kofft_hip_stft_rows_f32 /
 * kofft_hip_dev_stft_rows_f32 (plus rows * frames * K too large -> UNSUPPORTED); out is dense rows * frames * K complex, 8-byte
 * aligned, and out[r][f][k], k < K, has exactly the bits the rows call writes to [r][f][k] -- the prefix of the full frame, for
 * every window length that call takes; nothing of bins K .. win_len - 1 is written anywhere.  Window lengths that are not a power
 * of two go through scratch the context owns (at most 512 MiB, until kofft_hip_release_scratch / destroy).
 * Inverse: half is rows * frames * K complex and is only read.  Every frame is completed to F[k] = half[k] for k < K,
 * F[k] = (half[win_len - k].re, -half[win_len - k].im) for K <= k < win_len (the imaginary parts of bins 0 and win_len / 2 are
 * used as given), and the result is exactly kofft_hip_istft_parallel_rows_f32 of F: output (rows * out_len) is accumulated into
 * and normalised, a sample whose window-square sum is <= 1e-8 becomes 0.  Checks: those of the parallel rows form, in its order.
 * Both device forms work through scratch the context owns, like kofft_hip_dev_istft_parallel_rows_f32. */
int kofft_hip_stft_onesided_f32(kofft_hip_ctx *ctx, const float *signal, size_t rows, size_t len, size_t row_stride,
                                const float *window, size_t win_len, size_t hop, float *out, size_t frames);
int kofft_hip_dev_stft_onesided_f32(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len,
                                    size_t row_stride, const float *d_window, size_t win_len, size_t hop,
                                    float *d_out, size_t frames);
int kofft_hip_istft_onesided_f32(kofft_hip_ctx *ctx, const float *half, size_t rows, size_t frames,
                                 const float *window, size_t win_len, size_t hop, float *output, size_t out_len);
int kofft_hip_dev_istft_onesided_f32(kofft_hip_ctx *ctx, const float *d_half, size_t rows, size_t frames,
                                     const float *d_window, size_t win_len, size_t hop, float *d_output,
                                     size_t out_len);

/* ---- 2-D / 3-D FFT (SURVEY 8f "next" row 3) ----------------------------------------
 * ndfft::fft2d_inplace (ndfft.rs:74-101) with depth == 1: FftImpl::fft on every row (length cols), then
 * FftImpl::fft_strided down every column (length rows, stride cols).  ndfft::fft3d_inplace
 * (ndfft.rs:114-155) with depth > 1: z axis (stride rows*cols), y axis (stride cols), x axis (rows).
 * data: depth*rows*cols complex, row-major, in place.  Any zero dimension -> KOFFT_OK (nothing to do).
 * The reference's scratch-length checks belong to the host mirrors (they take the scratch slices).
 * inverse != 0 applies ifft / ifft_strided along the same axes in the same order. */
int kofft_hip_fftnd_c32(kofft_hip_ctx *ctx, float *data, size_t depth, size_t rows, size_t cols, int inverse);
int kofft_hip_fftnd_c64(kofft_hip_ctx *ctx, double *data, size_t depth, size_t rows, size_t cols, int inverse);
int kofft_hip_fftnd_c32_dev(kofft_hip_ctx *ctx, float *d_data, size_t depth, size_t rows, size_t cols, int inverse);
int kofft_hip_fftnd_c64_dev(kofft_hip_ctx *ctx, double *d_data, size_t depth, size_t rows, size_t cols, int inverse);

/* ---- multi-GPU ------------------------------------------------------
 * stft::parallel (stft.rs:232-263) runs rayon over frames; fft::batch (fft.rs:2156-2175) and the row loop around
 * RfftPlanner::rfft_with_scratch (rfft.rs:264-282) run over independent transforms.  The device analogue is ONE process
 * that owns `ngpu` devices (one context + one stream per device): device r works on the contiguous block
 * [r*ceil(U/G), min((r+1)*ceil(U/G), U)) of the U frames / transforms / rows.  STFT: from its own slice of the signal (the
 * slice plus the win_len-hop halo, cut on the host: no halo exchange).  `allgather` != 0 adds BASELINE config #4's exchange:
 * one RCCL ncclAllGather per device (ncclCommInitAll communicators, ncclGroupStart/End, in place) after which every device
 * holds the whole spectrogram in ceil(F/G)-frame slots.  RCCL is bound at run time (dlopen); without it allgather returns
 * KOFFT_ERR_RCCL and everything else still works.
 *
 * HOST-pointer entries return when the result is in the caller's memory.  Each device has its own worker thread that
 * uploads, launches and downloads that device's block (copies from pageable memory block the issuing thread: one thread per
 * device is what lets the G PCIe links run together); only the grouped all-gather is issued by the calling thread.
 * DEVICE-pointer entries (*_dev) take one device pointer per device (arrays of ngpu pointers, entry r valid on device r),
 * enqueue on the per-device streams from the calling thread and return WITHOUT synchronising
 * (kofft_hip_multi_synchronize, or a stream of kofft_hip_multi_context).  The calling thread's current device is left as found.
 *
 * kofft_hip_stft_f32_multi: one call, host pointers in and out; checks = stft::stft's (hop == 0 -> INVALID_HOP_SIZE,
 * frames < ceil(len/hop) -> MISMATCHED_LENGTHS, win_len == 0 -> EMPTY_INPUT), ngpu <= 0 -> INVALID_VALUE.
 * out: frames * win_len complex.  The handle form keeps contexts, buffers, threads and communicators across calls:
 *   kofft_hip_multi_create(ngpu, devices (NULL: 0..ngpu-1), &m)
 *   kofft_hip_multi_stft_f32(m, ..., out (host or NULL), frames, allgather, d_out_per_gpu (NULL or ngpu slots))
 *     d_out_per_gpu[r] receives device r's buffer (owned by m, valid until the next call): its shard, or with allgather
 *     the gathered [G*ceil(F/G), win_len] spectrogram (first `frames` rows are the STFT, the rest zero).
 *   kofft_hip_multi_stft_f32_dev(m, d_signal_per_gpu, len, d_window_per_gpu, win_len, hop, frames, allgather, d_out_per_gpu)
 *     device r holds ITS SLICE of the `len`-sample signal, kofft_hip_multi_stft_slice(m, len, win_len, hop, frames, r, &first,
 *     &count) samples starting at sample `first` (an empty slice may be NULL), and a copy of the window.  d_out_per_gpu is
 *     in/out: a non-NULL entry is the caller's buffer for device r (count_r * win_len complex, or G*ceil(F/G)*win_len with
 *     allgather); a NULL entry is replaced by a buffer owned by m.
 *   kofft_hip_multi_fft_c32 / _c64: fft::batch with the batch in G contiguous blocks, in place, no exchange;
 *   kofft_hip_multi_rfft_f32: rows of n reals -> rows of n/2+1 complex, optional window (BASELINE config #3's shape);
 *   their *_dev twins: d_*_per_gpu[r] points at device r's block of kofft_hip_multi_shard(m, batch, r, ..) rows.
 *   kofft_hip_multi_shard(m, total, rank, &first, &count): the partition above, for callers that place their own data.
 *   kofft_hip_multi_context(m, rank, &ctx, &hip_stream): device r's context and stream (either may be NULL), to order
 *     caller work against the handle's or to call any single-device entry on that device.
 *   kofft_hip_multi_last_timing_ex: the slowest device's time in each phase of the last call, from HIP events on the
 *     per-device streams: upload (host forms), kernel (kernels only -- no copy inside), gather, download (host forms), and
 *     the host forms' wall time from entry to return.  Waits for a *_dev call's events.  Phases a call did not have are 0.
 *   kofft_hip_multi_last_timing (round-2 signature): compute_ms = kernel_ms above, gather_ms. */
typedef struct kofft_hip_multi kofft_hip_multi;
int kofft_hip_multi_create(int ngpu, const int *devices, kofft_hip_multi **out);
int kofft_hip_multi_destroy(kofft_hip_multi *m);
const char *kofft_hip_multi_last_error(const kofft_hip_multi *m);
int kofft_hip_multi_ngpu(const kofft_hip_multi *m);
int kofft_hip_multi_shard(const kofft_hip_multi *m, size_t total, int rank, size_t *first, size_t *count);
int kofft_hip_multi_stft_slice(const kofft_hip_multi *m, size_t len, size_t win_len, size_t hop, size_t frames, int rank,
                               size_t *first_sample, size_t *count);
int kofft_hip_multi_context(const kofft_hip_multi *m, int rank, kofft_hip_ctx **ctx, void **hip_stream);
int kofft_hip_multi_synchronize(kofft_hip_multi *m);
int kofft_hip_multi_last_timing(const kofft_hip_multi *m, float *compute_ms, float *gather_ms);
/* The exchange of the STFT spectra (BASELINE config #4; the device analogue of collecting stft::parallel's frames, stft.rs:232-263)
 * has two forms over the same partition and the same buffers: RCCL (one grouped in-place ncclAllGather per device) and DIRECT
 * (every device pushes its slot to every peer with hipMemcpyPeerAsync on a stream per peer: no RCCL needed, and the direct
 * pattern on point-to-point xGMI whatever RCCL would choose).  Default RCCL, or KOFFT_HIP_MULTI_GATHER=direct at creation;
 * `last` = the form the last call ran (0: it had no exchange). */
#define KOFFT_MULTI_GATHER_RCCL 1
#define KOFFT_MULTI_GATHER_DIRECT 2
int kofft_hip_multi_set_gather(kofft_hip_multi *m, int mode);
int kofft_hip_multi_gather_mode(const kofft_hip_multi *m, int *configured, int *last);
int kofft_hip_multi_last_timing_ex(const kofft_hip_multi *m, float *upload_ms, float *kernel_ms, float *gather_ms,
                                   float *download_ms, float *wall_ms);
int kofft_hip_multi_stft_f32(kofft_hip_multi *m, const float *signal, size_t len, const float *window, size_t win_len,
                             size_t hop, float *out, size_t frames, int allgather, float **d_out_per_gpu);
int kofft_hip_multi_stft_f32_dev(kofft_hip_multi *m, const float *const *d_signal_per_gpu, size_t len,
                                 const float *const *d_window_per_gpu, size_t win_len, size_t hop, size_t frames, int allgather,
                                 float **d_out_per_gpu);
int kofft_hip_stft_f32_multi(int ngpu, const float *signal, size_t len, const float *window, size_t win_len,
                             size_t hop, float *out, size_t frames, int allgather);
int kofft_hip_multi_fft_c32(kofft_hip_multi *m, float *data, size_t n, size_t batch, int inverse);
int kofft_hip_multi_fft_c64(kofft_hip_multi *m, double *data, size_t n, size_t batch, int inverse);
int kofft_hip_multi_rfft_f32(kofft_hip_multi *m, const float *in, float *out, const float *window, size_t n, size_t batch);
int kofft_hip_multi_fft_c32_dev(kofft_hip_multi *m, float *const *d_data_per_gpu, size_t n, size_t batch, int inverse);
int kofft_hip_multi_fft_c64_dev(kofft_hip_multi *m, double *const *d_data_per_gpu, size_t n, size_t batch, int inverse);
int kofft_hip_multi_rfft_f32_dev(kofft_hip_multi *m, const float *const *d_in_per_gpu, float *const *d_out_per_gpu,
                                 const float *const *d_window_per_gpu, size_t n, size_t batch);

#ifdef __cplusplus
}
#endif
#endif /* KOFFT_HIP_H */
