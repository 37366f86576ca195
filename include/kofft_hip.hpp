// kofft_hip.hpp -- C++17 host mirror of kofft's operator interface for the hot path, on top of the C ABI
// (kofft_hip.h).  The reference is a Rust crate and the build image has no Rust toolchain, so this header plays
// the role the Rust shim (integration/rust/kofft-hip) plays for Rust callers: same names, same argument meaning,
// same error variants and validation order, so that tests read like the reference's own.
//
//   kofft::FftError, FftStrategy                 fft.rs:447-463
//   kofft::Complex<T>, Complex32, Complex64      num.rs:105-110, 232-233   (#[repr(C)] {re, im})
//   kofft::FftImpl<T>  (abstract)                fft.rs:466-587
//   kofft::HipFftImpl<T>  ~ ScalarFftImpl<T>     fft.rs:600-613 + RealFftImpl blanket methods (rfft.rs:775-837)
//   kofft::FftPlanner<T>, RfftPlanner<T>         fft.rs:332-445, rfft.rs:194-338
//   kofft::batch / batch_inverse / multi_channel fft.rs:2156-2191
//   kofft::stft / istft / parallel / frame / StftStream  stft.rs:76-156, 232-263, 355-372, 160-206
//   kofft::hann                                  window.rs:24-28
//   kofft::HipFftImpl<T>::fft_split / ifft_split, SplitComplex<T>, ComplexVec, fft_split_complex, fft_complex_vec
//                                                fft.rs:1365-1439, 2081-2153, num.rs:236-308 (the planes go to the device as they are)
//   kofft::HipFftImpl<float>::dct2               DctPlanner::plan_dct2, dct.rs:61-105
//   kofft::HipFftImpl<float>::hilbert_analytic   hilbert::hilbert_analytic, hilbert.rs:13-47
//   kofft::HipFftImpl<float>::real_cepstrum      cepstrum::real_cepstrum, cepstrum.rs:12-33
//   kofft::HipFftImpl<float>::mel_filterbank / mfcc, kofft::mel_bins   cepstrum::mel_filterbank / mfcc / mfcc_batch, cepstrum.rs:36-98
//                                                (the filter edges are an argument; mel_bins computes the reference-shaped ones)
//   kofft::HipFftImpl<float>::stft_mel / stft_mfcc   stft_magnitudes -> mel_filterbank (-> logf -> dct2) of rows of signals in one call,
//                                                the magnitudes never leaving the device (no counterpart in the reference: its pipeline)
//   kofft::HipFftImpl<float>::magnitude_to_db / db_scale / spectrogram_render, kofft::log_bin_map / map_color_u8
//   kofft::HipFftImpl<float>::stft_picture / stft_picture_dev   audio -> stft_magnitudes -> the row's, the running (web-spectrogram's
//                                                compute_frame) or a given maximum -> one picture per row, in one call
//                                                visual::spectrogram's colour helpers, visual/spectrogram.rs:96-234 (log10 is the libm
//                                                crate's log10f; Viridis / Plasma / Inferno are InvalidValue)
//   kofft::HipFftImpl<float>::dct_direct         dct::dct1..dct4, dct.rs:108-176 (the direct sums)
//   kofft::HipFftImpl<float>::dst_direct         dst::dst1..dst4, dst.rs:89-146
//   kofft::HipFftImpl<float>::dwt / idwt         wavelet::<name>_forward / _inverse, wavelet.rs:12-33, 154-535
//   kofft::HipFftImpl<float>::dwt_multi / idwt_multi   wavelet::multi_level_forward / _inverse, wavelet.rs:54-84
//   kofft::HipFftImpl<float>::dht                hartley::dht / batch, hartley.rs:12-57
//   kofft::hamming / blackman / kaiser / tukey / bartlett / bohman / nuttall   window.rs:31-61, window_more.rs:13-64
//
// Result<(), FftError> becomes kofft::Result (is_ok / is_err / unwrap / unwrap_err).  A negative C-ABI status
// (HIP failure, unsupported length) has no FftError variant: it throws kofft::DeviceError, the C++ analogue of
// the Rust shim's panic.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "kofft_hip.h"

namespace kofft {

enum class FftError : int {  // fft.rs:447-454, discriminant + 1 == C ABI status
    EmptyInput = 1,
    NonPowerOfTwoNoStd = 2,
    MismatchedLengths = 3,
    InvalidStride = 4,
    InvalidHopSize = 5,
    InvalidValue = 6,
};

enum class FftStrategy { Radix2, Radix4, SplitRadix, Auto };  // fft.rs:456-463

struct DeviceError : std::runtime_error {
    int status;
    DeviceError(int s, const std::string &detail)
        : std::runtime_error(std::string("kofft_hip status ") + std::to_string(s) + ": " + kofft_hip_strerror(s) +
                             (detail.empty() ? "" : " [" + detail + "]")),
          status(s)
    {
    }
};

class Result {
public:
    Result() : code_(0) {}
    explicit Result(FftError e) : code_(static_cast<int>(e)) {}
    static Result Ok() { return Result(); }
    static Result Err(FftError e) { return Result(e); }
    bool is_ok() const { return code_ == 0; }
    bool is_err() const { return code_ != 0; }
    void unwrap() const
    {
        if (code_ != 0) throw std::logic_error(std::string("called unwrap() on Err(") + kofft_hip_strerror(code_) + ")");
    }
    FftError unwrap_err() const
    {
        if (code_ == 0) throw std::logic_error("called unwrap_err() on Ok");
        return static_cast<FftError>(code_);
    }
    bool operator==(const Result &o) const { return code_ == o.code_; }

private:
    int code_;
};

template <typename T>
struct Complex {  // layout-compatible with T[2] (tests/complex_repr.rs)
    T re, im;
    Complex() : re(0), im(0) {}
    Complex(T r, T i) : re(r), im(i) {}
    static Complex zero() { return Complex(0, 0); }
    Complex add(Complex o) const { return Complex(re + o.re, im + o.im); }
    Complex sub(Complex o) const { return Complex(re - o.re, im - o.im); }
    Complex mul(Complex o) const { return Complex(re * o.re - im * o.im, re * o.im + im * o.re); }  // num.rs:161-166
    bool operator==(const Complex &o) const { return re == o.re && im == o.im; }
};
using Complex32 = Complex<float>;
using Complex64 = Complex<double>;
static_assert(sizeof(Complex32) == 2 * sizeof(float) && sizeof(Complex64) == 2 * sizeof(double), "repr(C) layout");

namespace detail {
template <typename T> struct Abi;
template <> struct Abi<float> {
    static int fft(kofft_hip_ctx *c, float *d, size_t n, size_t b, int inv) { return kofft_hip_fft_c32(c, d, n, b, inv); }
    static int strided(kofft_hip_ctx *c, float *d, size_t len, size_t st, size_t n, int inv) { return kofft_hip_fft_c32_strided(c, d, len, st, n, inv); }
    static int rfft(kofft_hip_ctx *c, const float *i, float *o, const float *w, size_t n, size_t b) { return kofft_hip_rfft_f32(c, i, o, w, n, b); }
    static int irfft(kofft_hip_ctx *c, const float *i, float *o, size_t n, size_t b) { return kofft_hip_irfft_f32(c, i, o, n, b); }
    static int twiddles(size_t n, float *o) { return kofft_hip_twiddles_f32(n, o); }
    static int rfft_table(size_t m, float *o) { return kofft_hip_rfft_table_f32(m, o); }
    static int fftnd(kofft_hip_ctx *c, float *d, size_t dp, size_t r, size_t cl, int inv) { return kofft_hip_fftnd_c32(c, d, dp, r, cl, inv); }
    static int radix4(kofft_hip_ctx *c, float *d, size_t n, size_t b) { return kofft_hip_fft_radix4_c32(c, d, n, b); }
    static int iradix4(kofft_hip_ctx *c, float *d, size_t n, size_t b) { return kofft_hip_ifft_radix4_c32(c, d, n, b); }
    static int split(kofft_hip_ctx *c, float *re, float *im, size_t n, size_t b, int inv) { return kofft_hip_fft_split_c32(c, re, im, n, b, inv); }
    static int split_dev(kofft_hip_ctx *c, const float *ri, const float *ii, float *ro, float *io, size_t n, size_t b, int inv)
    {
        return kofft_hip_dev_fft_split_c32(c, ri, ii, ro, io, n, b, inv);
    }
};
template <> struct Abi<double> {
    static int fft(kofft_hip_ctx *c, double *d, size_t n, size_t b, int inv) { return kofft_hip_fft_c64(c, d, n, b, inv); }
    static int strided(kofft_hip_ctx *c, double *d, size_t len, size_t st, size_t n, int inv) { return kofft_hip_fft_c64_strided(c, d, len, st, n, inv); }
    static int rfft(kofft_hip_ctx *c, const double *i, double *o, const double *w, size_t n, size_t b) { return kofft_hip_rfft_f64(c, i, o, w, n, b); }
    static int irfft(kofft_hip_ctx *c, const double *i, double *o, size_t n, size_t b) { return kofft_hip_irfft_f64(c, i, o, n, b); }
    static int twiddles(size_t n, double *o) { return kofft_hip_twiddles_f64(n, o); }
    static int rfft_table(size_t m, double *o) { return kofft_hip_rfft_table_f64(m, o); }
    static int fftnd(kofft_hip_ctx *c, double *d, size_t dp, size_t r, size_t cl, int inv) { return kofft_hip_fftnd_c64(c, d, dp, r, cl, inv); }
    static int radix4(kofft_hip_ctx *c, double *d, size_t n, size_t b) { return kofft_hip_fft_radix4_c64(c, d, n, b); }
    static int iradix4(kofft_hip_ctx *c, double *d, size_t n, size_t b) { return kofft_hip_ifft_radix4_c64(c, d, n, b); }
    static int split(kofft_hip_ctx *c, double *re, double *im, size_t n, size_t b, int inv) { return kofft_hip_fft_split_c64(c, re, im, n, b, inv); }
    static int split_dev(kofft_hip_ctx *c, const double *ri, const double *ii, double *ro, double *io, size_t n, size_t b, int inv)
    {
        return kofft_hip_dev_fft_split_c64(c, ri, ii, ro, io, n, b, inv);
    }
};
}  // namespace detail

// trait FftImpl<T> (fft.rs:466-587): the required methods are pure virtual, the provided ones have the
// reference's default bodies.
template <typename T>
class FftImpl {
public:
    using C = Complex<T>;
    virtual ~FftImpl() = default;
    virtual Result fft(std::vector<C> &input) const = 0;
    virtual Result ifft(std::vector<C> &input) const = 0;
    virtual Result fft_strided(std::vector<C> &input, size_t stride, std::vector<C> &scratch) const = 0;
    virtual Result ifft_strided(std::vector<C> &input, size_t stride, std::vector<C> &scratch) const = 0;
    virtual Result fft_out_of_place_strided(const std::vector<C> &input, size_t in_stride, std::vector<C> &output,
                                            size_t out_stride) const = 0;
    virtual Result ifft_out_of_place_strided(const std::vector<C> &input, size_t in_stride, std::vector<C> &output,
                                             size_t out_stride) const = 0;
    virtual Result fft_with_strategy(std::vector<C> &input, FftStrategy strategy) const = 0;

    Result fft_out_of_place(const std::vector<C> &input, std::vector<C> &output) const  // fft.rs:469-479
    {
        if (input.size() != output.size()) return Result::Err(FftError::MismatchedLengths);
        output = input;
        return fft(output);
    }
    Result ifft_out_of_place(const std::vector<C> &input, std::vector<C> &output) const  // fft.rs:480-490
    {
        if (input.size() != output.size()) return Result::Err(FftError::MismatchedLengths);
        output = input;
        return ifft(output);
    }
    virtual Result fft_split(std::vector<T> &re, std::vector<T> &im) const  // fft.rs:556-570
    {
        if (re.size() != im.size()) return Result::Err(FftError::MismatchedLengths);
        std::vector<C> buf(re.size());
        for (size_t i = 0; i < re.size(); ++i) buf[i] = C(re[i], im[i]);
        Result r = fft(buf);
        if (r.is_err()) return r;
        for (size_t i = 0; i < re.size(); ++i) { re[i] = buf[i].re; im[i] = buf[i].im; }
        return Result::Ok();
    }
    virtual Result ifft_split(std::vector<T> &re, std::vector<T> &im) const  // fft.rs:572-586
    {
        if (re.size() != im.size()) return Result::Err(FftError::MismatchedLengths);
        std::vector<C> buf(re.size());
        for (size_t i = 0; i < re.size(); ++i) buf[i] = C(re[i], im[i]);
        Result r = ifft(buf);
        if (r.is_err()) return r;
        for (size_t i = 0; i < re.size(); ++i) { re[i] = buf[i].re; im[i] = buf[i].im; }
        return Result::Ok();
    }
};

// Drop-in for ScalarFftImpl<T>: one device context per instance, not shared between threads (fft.rs:589-605).
template <typename T>
class HipFftImpl : public FftImpl<T> {
public:
    using C = Complex<T>;
    explicit HipFftImpl(int device = 0)
    {
        int rc = kofft_hip_create(device, &ctx_);
        if (rc != 0) throw DeviceError(rc, "kofft_hip_create");
        const char *e = std::getenv("KOFFT_HIP_RADIX4_COMPAT");
        radix4_compat = !(e && e[0] == '0');
    }
    // fft_with_strategy(.., Radix4) reproduces the reference's fft_radix4 bytes (fft.rs:1356, 1455-1548; NOT a DFT from
    // n = 16): strict drop-in, ON by default since round 6.  KOFFT_HIP_RADIX4_COMPAT=0, or false here, opts out (the true
    // transform for every strategy).
    bool radix4_compat = true;
    static HipFftImpl default_() { return HipFftImpl(0); }
    ~HipFftImpl() override { if (ctx_) kofft_hip_destroy(ctx_); }
    HipFftImpl(const HipFftImpl &) = delete;
    HipFftImpl &operator=(const HipFftImpl &) = delete;
    HipFftImpl(HipFftImpl &&o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    kofft_hip_ctx *raw() const { return ctx_; }

    Result fft(std::vector<C> &input) const override { return st(detail::Abi<T>::fft(ctx_, fp(input), input.size(), 1, 0)); }
    Result ifft(std::vector<C> &input) const override { return st(detail::Abi<T>::fft(ctx_, fp(input), input.size(), 1, 1)); }
    Result stockham_fft(std::vector<C> &input) const { return fft(input); }  // fft.rs:634-640
    // fft.rs:1365-1439: the SoA entries, in place on the two planes through the C entry (no packing on the host); the bytes are
    // those of fft / ifft on re + i im
    Result fft_split(std::vector<T> &re, std::vector<T> &im) const override
    {
        if (re.size() != im.size()) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::split(ctx_, re.data(), im.data(), re.size(), 1, 0));
    }
    Result ifft_split(std::vector<T> &re, std::vector<T> &im) const override
    {
        if (re.size() != im.size()) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::split(ctx_, re.data(), im.data(), re.size(), 1, 1));
    }
    // added: every row of two contiguous planes of batch * n reals, in place
    Result fft_split_batch(std::vector<T> &re, std::vector<T> &im, size_t n, bool inverse = false) const
    {
        if (re.size() != im.size() || (n != 0 && re.size() % n != 0)) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::split(ctx_, re.data(), im.data(), n, n == 0 ? 1 : re.size() / n, inverse ? 1 : 0));
    }
    // added: device pointers, asynchronous on the context's stream; an output plane may be its own input
    Result fft_split_dev(const T *d_re_in, const T *d_im_in, T *d_re_out, T *d_im_out, size_t n, size_t batch, bool inverse = false) const
    {
        return st(detail::Abi<T>::split_dev(ctx_, d_re_in, d_im_in, d_re_out, d_im_out, n, batch, inverse ? 1 : 0));
    }
    // false: every planar transform of this context through pack, n-point transform, unpack (the same bytes; A/B, tests)
    Result set_split_fused(bool on) const { return st(kofft_hip_set_split_fused(ctx_, on ? 1 : 0)); }
    Result fft_strided(std::vector<C> &input, size_t stride, std::vector<C> &scratch) const override
    {
        return st(detail::Abi<T>::strided(ctx_, fp(input), input.size(), stride, scratch.size(), 0));
    }
    Result ifft_strided(std::vector<C> &input, size_t stride, std::vector<C> &scratch) const override
    {
        return st(detail::Abi<T>::strided(ctx_, fp(input), input.size(), stride, scratch.size(), 1));
    }
    Result fft_out_of_place_strided(const std::vector<C> &input, size_t in_stride, std::vector<C> &output,
                                    size_t out_stride) const override
    {
        return oop_strided(input, in_stride, output, out_stride, false);
    }
    Result ifft_out_of_place_strided(const std::vector<C> &input, size_t in_stride, std::vector<C> &output,
                                     size_t out_stride) const override
    {
        return oop_strided(input, in_stride, output, out_stride, true);
    }
    // fft.rs:1337-1363.  Radix2 / SplitRadix / Auto run the Stockham path (fft and stockham_fft agree for n >= 2); Radix4
    // runs fft_radix4 (fft.rs:1356) like the reference -- not a DFT from n = 16 (its digit-reversal loop is wrong; DESIGN.md
    // section 1), but a drop-in returns the reference's bytes (kofft_hip_fft_radix4_*).  radix4_compat = false opts out.
    Result fft_with_strategy(std::vector<C> &input, FftStrategy strategy) const override
    {
        if (input.empty()) return Result::Err(FftError::EmptyInput);
        if (input.size() == 1) return Result::Ok();
        if (strategy == FftStrategy::Radix4 && radix4_compat) return fft_radix4(input);
        return fft(input);
    }
    // ScalarFftImpl::fft_radix4 (fft.rs:1455-1548), the reference's bytes
    Result fft_radix4(std::vector<C> &input) const { return st(detail::Abi<T>::radix4(ctx_, fp(input), input.size(), 1)); }
    // FftPlan::ifft's loop around that arm (fft.rs:2040-2055): conj, fft_radix4, conj * 1/(n as f32), on the device
    Result ifft_radix4(std::vector<C> &input) const
    {
        if (input.empty()) return Result::Err(FftError::EmptyInput);
        return st(detail::Abi<T>::iradix4(ctx_, fp(input), input.size(), 1));
    }

    // RealFftImpl<T> blanket methods (rfft.rs:780-833); checks in rfft_direct's order (rfft.rs:433-443)
    Result rfft_with_scratch(std::vector<T> &input, std::vector<C> &output, std::vector<C> &scratch) const
    {
        const size_t n = input.size();
        if (n == 0) return Result::Err(FftError::EmptyInput);
        if (n % 2 != 0) return Result::Err(FftError::InvalidValue);
        if (output.size() != n / 2 + 1 || scratch.size() < n / 2) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::rfft(ctx_, input.data(), fp(output), nullptr, n, 1));
    }
    Result rfft(std::vector<T> &input, std::vector<C> &output) const
    {
        std::vector<C> scratch(input.size() / 2);
        return rfft_with_scratch(input, output, scratch);
    }
    Result irfft_with_scratch(std::vector<C> &input, std::vector<T> &output, std::vector<C> &scratch) const
    {
        const size_t n = output.size();
        if (n == 0) return Result::Err(FftError::EmptyInput);
        if (n % 2 != 0) return Result::Err(FftError::InvalidValue);
        if (input.size() != n / 2 + 1 || scratch.size() < n / 2) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::irfft(ctx_, reinterpret_cast<const T *>(input.data()), output.data(), n, 1));
    }
    Result irfft(std::vector<C> &input, std::vector<T> &output) const
    {
        std::vector<C> scratch(output.size() / 2);
        return irfft_with_scratch(input, output, scratch);
    }
    // DctPlanner::plan_dct2 (dct.rs:61-105), f32 only like the reference: `batch` contiguous rows of n reals in and out.
    // Checks in dct2_with_table's order: MismatchedLengths (dct.rs:68-70), then the rfft's EmptyInput (rfft.rs:434).
    Result dct2(const std::vector<float> &input, std::vector<float> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "dct2 is f32-only (dct.rs:6)");
        if (batch == 0 || input.size() % batch != 0 || output.size() != input.size()) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        if (n == 0) return Result::Err(FftError::EmptyInput);
        return st(kofft_hip_dct2_f32(ctx_, input.data(), output.data(), n, batch));
    }
    // hilbert::hilbert_analytic (hilbert.rs:13-47), f32 only like the reference: `batch` contiguous rows of n reals in, rows of n complex
    // out.  MismatchedLengths for rows that do not divide the input or an output of another size; then the reference's EmptyInput and
    // NonPowerOfTwoNoStd (hilbert.rs:14-19).
    Result hilbert_analytic(const std::vector<float> &input, std::vector<C> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "hilbert_analytic is f32-only (hilbert.rs:13)");
        if (batch == 0 || input.size() % batch != 0 || output.size() != input.size()) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        if (n == 0) return Result::Err(FftError::EmptyInput);
        if (n & (n - 1)) return Result::Err(FftError::NonPowerOfTwoNoStd);
        return st(kofft_hip_hilbert_f32(ctx_, input.data(), reinterpret_cast<float *>(output.data()), n, batch));
    }
    // cepstrum::real_cepstrum (cepstrum.rs:12-33), f32 only like the reference: `batch` contiguous rows of n reals in, rows of n reals
    // out.  MismatchedLengths for rows that do not divide the input or an output of another size; then the reference's EmptyInput and
    // NonPowerOfTwoNoStd (cepstrum.rs:13-18).  input and output may be the same vector.
    Result real_cepstrum(const std::vector<float> &input, std::vector<float> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "real_cepstrum is f32-only (cepstrum.rs:12)");
        if (batch == 0 || input.size() % batch != 0 || output.size() != input.size()) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        if (n == 0) return Result::Err(FftError::EmptyInput);
        if (n & (n - 1)) return Result::Err(FftError::NonPowerOfTwoNoStd);
        return st(kofft_hip_cepstrum_f32(ctx_, input.data(), output.data(), n, batch));
    }
    // Overlap-save FFT convolution of `rows` contiguous rows of x.size() / rows samples with h: nh taps for all rows (h.size() == nh)
    // or per row (h.size() == rows * nh).  out is resized to rows * count: values first .. first + count of each row's full result
    // of nx + nh - 1 values (count == SIZE_MAX: up to its end).  block: the power-of-two transform length >= nh, 0: the library's
    // choice (kofft_hip_convolve_block).  MismatchedLengths for rows that do not divide x or taps of another size; then the C
    // entry's checks in its order.
    Result convolve_rows(const std::vector<float> &x, const std::vector<float> &h, size_t nh, std::vector<float> &out, size_t rows = 1,
                         size_t block = 0, size_t first = 0, size_t count = SIZE_MAX) const
    {
        return convolve_impl(x, h, nh, out, rows, block, first, count, 0u);
    }
    // false: every convolution of this context through frames in the scratch, transform, multiply, inverse transform, gather (the
    // same bytes; A/B, tests)
    Result set_convolve_fused(bool on) const { return st(kofft_hip_set_convolve_fused(ctx_, on ? 1 : 0)); }
    // The cross-correlation of the same rows: convolve_rows with the taps reversed (numpy.correlate's "full" order for real data).
    Result correlate_rows(const std::vector<float> &x, const std::vector<float> &h, size_t nh, std::vector<float> &out, size_t rows = 1,
                          size_t block = 0, size_t first = 0, size_t count = SIZE_MAX) const
    {
        return convolve_impl(x, h, nh, out, rows, block, first, count, 1u);
    }
    // The fast DCT-IV, the MDCT and the IMDCT of rows (kofft_hip_dct4_fast_f32, kofft_hip_mdct_f32, kofft_hip_imdct_f32; DESIGN.md
    // 5.32), f32 only.  dct4_fast_rows: `rows` contiguous rows of x.size() / rows reals (an even length) in x, the same shape in out.
    // MismatchedLengths for rows that do not divide x; then the C entry's checks in its order.
    Result dct4_fast_rows(const std::vector<float> &x, std::vector<float> &out, size_t rows = 1) const
    {
        static_assert(std::is_same<T, float>::value, "dct4_fast_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0) return Result::Err(FftError::MismatchedLengths);
        out.resize(x.size());
        return st(kofft_hip_dct4_fast_f32(ctx_, x.data(), out.data(), x.size() / rows, rows));
    }
    // mdct_rows: `rows` contiguous signals of x.size() / rows samples, a window of 2N values, `frames` frames per row (SIZE_MAX:
    // ceil(nx / N) + 1) after `lead` virtual zeros (SIZE_MAX: N); out is resized to rows * frames * N unscaled coefficients.
    // MismatchedLengths for rows that do not divide x or a window of odd length, EmptyInput for an empty window or signal.
    Result mdct_rows(const std::vector<float> &x, const std::vector<float> &window, std::vector<float> &out, size_t rows = 1,
                     size_t lead = SIZE_MAX, size_t frames = SIZE_MAX) const
    {
        static_assert(std::is_same<T, float>::value, "mdct_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0 || window.size() % 2 != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows, n = window.size() / 2;
        if (nx == 0 || n == 0) return Result::Err(FftError::EmptyInput);
        if (lead == SIZE_MAX) lead = n;
        if (frames == SIZE_MAX) frames = (nx + n - 1) / n + 1;
        out.resize(rows * frames * n);
        float dummy = 0.0f;  // (frames == 0: the C entry returns before it looks at the pointer)
        return st(kofft_hip_mdct_f32(ctx_, x.data(), rows, nx, nx, window.data(), n, lead, out.empty() ? &dummy : out.data(), frames));
    }
    // imdct_rows: coef holds rows * frames * N coefficients, N = window.size() / 2; out is resized to rows * count samples, first ..
    // first + count of the (frames + 1) N overlap-added samples per row (count == SIZE_MAX: up to the end), each times scale (a
    // negative scale: 2 / N).  MismatchedLengths for a window of odd length or coef that is no whole number of rows of frames.
    Result imdct_rows(const std::vector<float> &coef, const std::vector<float> &window, std::vector<float> &out, size_t rows = 1,
                      float scale = -1.0f, size_t first = 0, size_t count = SIZE_MAX) const
    {
        static_assert(std::is_same<T, float>::value, "imdct_rows is f32-only");
        if (rows == 0 || window.size() % 2 != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t n = window.size() / 2;
        if (n == 0) return Result::Err(FftError::EmptyInput);
        if (coef.size() % (rows * n) != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t frames = coef.size() / (rows * n), full = (frames + 1) * n;
        if (count == SIZE_MAX) {
            if (first > full) return Result::Err(FftError::MismatchedLengths);
            count = full - first;
        }
        if (first > full || count > full - first) return Result::Err(FftError::MismatchedLengths);
        out.resize(rows * count);
        float dummy = 0.0f;  // (count == 0: the C entry returns before it looks at the pointer)
        return st(kofft_hip_imdct_f32(ctx_, coef.data(), rows, frames, window.data(), n, scale < 0.0f ? 2.0f / (float)n : scale,
                                      out.empty() ? &dummy : out.data(), first, count));
    }
    // false: every fast DCT-IV, MDCT and IMDCT of this context through fold / pre-twiddle into the scratch, transform, post-twiddle
    // (the same bytes; A/B, tests)
    Result set_mdct_fused(bool on) const { return st(kofft_hip_set_mdct_fused(ctx_, on ? 1 : 0)); }
    // The polyphase filter bank of rows, analysis and synthesis (kofft_hip_pfb_analysis_f32, kofft_hip_pfb_synthesis_f32; DESIGN.md
    // 5.34), f32 only.  pfb_analysis_rows: `rows` contiguous signals of x.size() / rows samples, taps.size() = T * channels taps, hop
    // `hop` (0: channels), `frames` frames per row (SIZE_MAX: ceil((nx + lead) / hop), every frame that reaches a sample) after `lead`
    // virtual zeros, `bins` bins per frame (SIZE_MAX: the one-sided channels / 2 + 1); out is resized to rows * frames * bins.
    // MismatchedLengths for rows that do not divide x, EmptyInput for no channels, taps or samples; then the C entry's checks in its order.
    Result pfb_analysis_rows(const std::vector<float> &x, const std::vector<float> &taps, size_t channels, std::vector<Complex<float>> &out,
                             size_t rows = 1, size_t hop = 0, size_t lead = 0, size_t frames = SIZE_MAX, size_t bins = SIZE_MAX) const
    {
        static_assert(std::is_same<T, float>::value, "pfb_analysis_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows;
        if (nx == 0 || channels == 0 || taps.empty()) return Result::Err(FftError::EmptyInput);
        if (hop == 0) hop = channels;
        if (frames == SIZE_MAX) frames = (nx + lead + hop - 1) / hop;
        if (bins == SIZE_MAX) bins = channels / 2 + 1;
        out.resize(rows * frames * bins);
        Complex<float> dummy{};  // (frames == 0: the C entry returns before it looks at the pointer)
        return st(kofft_hip_pfb_analysis_f32(ctx_, x.data(), rows, nx, nx, taps.data(), taps.size(), channels, hop, lead,
                                             reinterpret_cast<float *>(out.empty() ? &dummy : out.data()), frames, bins));
    }
    // pfb_synthesis_rows: spec holds rows * frames * bins bins, bins = channels or channels / 2 + 1; out is resized to rows * count
    // samples, first .. first + count of the (frames - 1) hop + taps.size() overlap-added samples per row (count == SIZE_MAX: up to
    // the end), each times scale.  EmptyInput for no channels or taps, InvalidValue for a bins that is neither form, MismatchedLengths
    // for spec that is no whole number of rows of frames or a window past the end.
    Result pfb_synthesis_rows(const std::vector<Complex<float>> &spec, const std::vector<float> &taps, size_t channels, size_t hop, size_t bins,
                              std::vector<float> &out, size_t rows = 1, float scale = 1.0f, size_t first = 0, size_t count = SIZE_MAX) const
    {
        static_assert(std::is_same<T, float>::value, "pfb_synthesis_rows is f32-only");
        if (channels == 0 || taps.empty()) return Result::Err(FftError::EmptyInput);
        if (bins != channels && !(channels % 2 == 0 && bins == channels / 2 + 1)) return Result::Err(FftError::InvalidValue);
        if (rows == 0 || spec.size() % (rows * bins) != 0) return Result::Err(FftError::MismatchedLengths);
        if (hop == 0) return Result::Err(FftError::InvalidHopSize);
        const size_t frames = spec.size() / (rows * bins), full = frames ? (frames - 1) * hop + taps.size() : 0;
        if (first > full) return Result::Err(FftError::MismatchedLengths);
        if (count == SIZE_MAX) count = full - first;
        if (count > full - first) return Result::Err(FftError::MismatchedLengths);
        out.resize(rows * count);
        float dummy = 0.0f;  // (count == 0: the C entry writes nothing)
        return st(kofft_hip_pfb_synthesis_f32(ctx_, reinterpret_cast<const float *>(spec.data()), rows, frames, bins, taps.data(), taps.size(),
                                              channels, hop, scale, out.empty() ? &dummy : out.data(), first, count));
    }
    // 1: the measured choice (the default); 0: every filter-bank call of this context through fold into the scratch, transform, prefix
    // copy / completion, inverse transform, real parts; 2: the fused kernels wherever they exist (the same bytes; A/B, tests)
    Result set_pfb_fused(int on) const { return st(kofft_hip_set_pfb_fused(ctx_, on)); }
    // kofft_hip_pfb_taps_f32, no device: the sinc x Kaiser prototype of taps_per_channel * channels taps, normalised to unit sum
    // (empty on an error, whose status goes to *err).
    static std::vector<float> pfb_taps(size_t channels, size_t taps_per_channel, double beta = 5.0, int *err = nullptr)
    {
        std::vector<float> taps(channels * taps_per_channel);
        float dummy = 0.0f;
        const int rc = kofft_hip_pfb_taps_f32(channels, taps_per_channel, beta, taps.empty() ? &dummy : taps.data());
        if (err) *err = rc;
        if (rc != KOFFT_OK) taps.clear();
        return taps;
    }
    // kofft_hip_pfb_reconstruction, no device: c and the worst deviation of the reconstruction condition of (h, g) at this hop
    static int pfb_reconstruction(const std::vector<float> &h, const std::vector<float> &g, size_t channels, size_t hop, double &c, double &worst)
    {
        if (h.size() != g.size()) return KOFFT_ERR_MISMATCHED_LENGTHS;
        return kofft_hip_pfb_reconstruction(h.data(), g.data(), h.size(), channels, hop, &c, &worst);
    }
    // Overlap-save FFT convolution of `rows` contiguous rows of x.size() / rows samples with every filter of a bank that the rows
    // share (kofft_hip_convolve_bank_f32): h holds h.size() / nh filters of nh taps, float or Complex<float>; each frame is
    // transformed once for the whole bank.  out is resized to rows * filters * count elements, [row][filter][count]: values first ..
    // first + count of each full result of nx + nh - 1 values (count == SIZE_MAX: up to its end).  Out picks the output kind:
    // std::vector<float> with magnitude == false the real parts, with magnitude == true the magnitudes; std::vector<Complex<float>>
    // the complex values (with magnitude == true: InvalidValue).  correlate: the taps reversed and complex ones conjugated (numpy.correlate's "full" order).
    // MismatchedLengths for rows that do not divide x or nh that does not divide h; then the C entry's checks in its order.
    template <typename Tap, typename Out>
    Result convolve_bank_rows(const std::vector<float> &x, const std::vector<Tap> &h, size_t nh, std::vector<Out> &out, size_t rows = 1,
                              size_t block = 0, size_t first = 0, size_t count = SIZE_MAX, bool correlate = false,
                              bool magnitude = false) const
    {
        static_assert(std::is_same<T, float>::value, "convolve_bank_rows is f32-only");
        static_assert(std::is_same<Tap, float>::value || std::is_same<Tap, Complex<float>>::value, "taps: float or Complex<float>");
        static_assert(std::is_same<Out, float>::value || std::is_same<Out, Complex<float>>::value, "out: float or Complex<float>");
        constexpr bool complex_out = std::is_same<Out, Complex<float>>::value;
        if (complex_out && magnitude) return Result::Err(FftError::InvalidValue);
        if (rows == 0 || x.size() % rows != 0 || (nh != 0 && h.size() % nh != 0)) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows;
        if (nx == 0 || nh == 0) return Result::Err(FftError::EmptyInput);
        const size_t filters = h.size() / nh, full = nx + nh - 1;
        if (count == SIZE_MAX) {
            if (first > full) return Result::Err(FftError::MismatchedLengths);
            count = full - first;
        }
        if (first > full || count > full - first) return Result::Err(FftError::MismatchedLengths);
        out.resize(rows * filters * count);
        const unsigned flags = (correlate ? KOFFT_HIP_BANK_CORRELATE : 0u) |
                               (std::is_same<Tap, float>::value ? 0u : KOFFT_HIP_BANK_COMPLEX_TAPS) |
                               (complex_out ? KOFFT_HIP_BANK_OUT_COMPLEX : magnitude ? KOFFT_HIP_BANK_OUT_MAGNITUDE : KOFFT_HIP_BANK_OUT_REAL);
        Out dummy{};  // (no filters or count == 0: the C entry returns before it looks at the pointers)
        const float none = 0.0f;
        return st(kofft_hip_convolve_bank_f32(ctx_, x.data(), rows, nx, h.empty() ? &none : reinterpret_cast<const float *>(h.data()),
                                              filters, nh, block, flags, out.empty() ? static_cast<void *>(&dummy) : out.data(), first,
                                              count));
    }
    // false: every filter-bank convolution of this context through frames in the scratch transformed once, then per filter multiply,
    // inverse transform, gather (the same bytes; A/B, tests)
    Result set_convolve_bank_fused(bool on) const { return st(kofft_hip_set_convolve_bank_fused(ctx_, on ? 1 : 0)); }
    // Polyphase resampling of `rows` contiguous rows of x.size() / rows samples through the taps h (kofft_hip_resample_f32): out is
    // resized to rows * count values, output m of a row at up-sampled time t0 + m * down, in the arithmetic the C header fixes.  count
    // SIZE_MAX: every output from t0 to the end of the full result of (nx - 1) * up + h.size() values (scipy.signal.upfirdn's length at
    // t0 = 0).  MismatchedLengths for rows that do not divide x; then the C entry's checks in its order.
    Result resample_rows(const std::vector<float> &x, const std::vector<float> &h, size_t up, size_t down, std::vector<float> &out,
                         size_t rows = 1, size_t t0 = 0, size_t count = SIZE_MAX) const
    {
        static_assert(std::is_same<T, float>::value, "resample_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows, nh = h.size();
        if (count == SIZE_MAX) {
            if (nx == 0 || nh == 0) return Result::Err(FftError::EmptyInput);
            if (up == 0 || down == 0) return Result::Err(FftError::InvalidValue);
            size_t full_up = 0;
            if (__builtin_mul_overflow(nx - 1, up, &full_up) || __builtin_add_overflow(full_up, nh, &full_up))
                return st(KOFFT_ERR_UNSUPPORTED);
            count = t0 < full_up ? (full_up - t0 - 1) / down + 1 : 0;
        }
        size_t total = 0;
        if (__builtin_mul_overflow(rows, count, &total)) return st(KOFFT_ERR_UNSUPPORTED);
        out.assign(total, 0.0f);
        float dummy = 0.0f;
        return st(kofft_hip_resample_f32(ctx_, x.data(), rows, nx, h.data(), nh, up, down, t0, out.empty() ? &dummy : out.data(), count));
    }
    // 1: the measured choice (the default), 0: every resampling call of this context on the plain kernel, 2: the tiled kernel wherever
    // its tables fit (the same bytes; A/B, tests)
    Result set_resample_tiled(int mode) const { return st(kofft_hip_set_resample_tiled(ctx_, mode)); }
    // kofft_hip_resample_taps_f32, no device: scipy.signal.resample_poly's default filter for up / down (2 * zeros * max(up, down) + 1
    // taps).  Returns an empty vector and sets `err` on an error.
    static std::vector<float> resample_taps(size_t up, size_t down, size_t zeros = 10, double beta = 5.0, int *err = nullptr)
    {
        size_t nh = 0;
        int rc = kofft_hip_resample_taps_f32(up, down, zeros, beta, nullptr, &nh);
        std::vector<float> taps;
        if (!rc) {
            taps.resize(nh);
            rc = kofft_hip_resample_taps_f32(up, down, zeros, beta, taps.data(), &nh);
        }
        if (err) *err = rc;
        if (rc) taps.clear();
        return taps;
    }
    // IIR filtering of `rows` contiguous rows of x.size() / rows samples by the cascade of sos.size() / 6 biquads (kofft_hip_sosfilt_f32:
    // b0 b1 b2 a0 a1 a2 per section, a0 == 1): out is resized to x.size() values, in the arithmetic the C header fixes.  zi: the initial
    // state [rows][sections][2], or null for zeros; zf: resized to rows * sections * 2 final-state values, or null for none; zf == zi
    // updates the state in place, and &out == &x filters in place.  reverse: every row is walked from its last sample.  MismatchedLengths
    // for rows that do not divide x, a sos that is no multiple of 6 values or a zi of another size; then the C entry's checks in its order.
    Result sosfilt_rows(const std::vector<float> &x, const std::vector<float> &sos, std::vector<float> &out, size_t rows = 1,
                        const std::vector<float> *zi = nullptr, std::vector<float> *zf = nullptr, bool reverse = false) const
    {
        static_assert(std::is_same<T, float>::value, "sosfilt_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0 || sos.size() % 6 != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows, sections = sos.size() / 6;
        size_t state = 0;
        if (__builtin_mul_overflow(rows, sections, &state) || __builtin_mul_overflow(state, (size_t)2, &state)) return st(KOFFT_ERR_UNSUPPORTED);
        if (zi && zi->size() != state) return Result::Err(FftError::MismatchedLengths);
        if (&out != &x) out.assign(x.size(), 0.0f);
        if (zf && zf != zi) zf->assign(state, 0.0f);
        float dummy = 0.0f;
        return st(kofft_hip_sosfilt_f32(ctx_, x.empty() ? &dummy : x.data(), rows, nx, sos.empty() ? &dummy : sos.data(), sections,
                                        zi && !zi->empty() ? zi->data() : nullptr, zf && !zf->empty() ? zf->data() : nullptr,
                                        reverse ? KOFFT_HIP_SOSFILT_REVERSE : 0u, out.empty() ? &dummy : out.data()));
    }
    // sosfilt_rows as a scan along time (kofft_hip_sosfilt_scan_f32): every row is cut into chunks of `chunk` samples (a multiple of
    // KOFFT_HIP_SOSFILT_TILE) that are filtered in parallel, in the scan's own bit-exact definition of the C header -- sosfilt_rows'
    // bits in the first chunk, others after it.  The arguments, sizes and errors of sosfilt_rows; chunk == 0 or no multiple of the tile:
    // InvalidValue.  scan_chunk: kofft_hip_sosfilt_scan_chunk's measured choice for a shape.
    Result sosfilt_scan_rows(const std::vector<float> &x, const std::vector<float> &sos, std::vector<float> &out, size_t chunk, size_t rows = 1,
                             const std::vector<float> *zi = nullptr, std::vector<float> *zf = nullptr, bool reverse = false) const
    {
        static_assert(std::is_same<T, float>::value, "sosfilt_scan_rows is f32-only");
        if (rows == 0 || x.size() % rows != 0 || sos.size() % 6 != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows, sections = sos.size() / 6;
        size_t state = 0;
        if (__builtin_mul_overflow(rows, sections, &state) || __builtin_mul_overflow(state, (size_t)2, &state)) return st(KOFFT_ERR_UNSUPPORTED);
        if (zi && zi->size() != state) return Result::Err(FftError::MismatchedLengths);
        if (&out != &x) out.assign(x.size(), 0.0f);
        if (zf && zf != zi) zf->assign(state, 0.0f);
        float dummy = 0.0f;
        return st(kofft_hip_sosfilt_scan_f32(ctx_, x.empty() ? &dummy : x.data(), rows, nx, sos.empty() ? &dummy : sos.data(), sections,
                                             zi && !zi->empty() ? zi->data() : nullptr, zf && !zf->empty() ? zf->data() : nullptr, chunk,
                                             reverse ? KOFFT_HIP_SOSFILT_REVERSE : 0u, out.empty() ? &dummy : out.data()));
    }
    static size_t sosfilt_scan_chunk(size_t rows, size_t nx, size_t sections)
    {
        size_t chunk = 0;
        (void)kofft_hip_sosfilt_scan_chunk(rows, nx, sections, &chunk);
        return chunk;
    }
    // 1: the measured choice (the default), 0: every sosfilt call of this context on the plain kernel, 2: the tiled kernel wherever it
    // exists (the same bytes; A/B, tests)
    Result set_sosfilt_tiled(int mode) const { return st(kofft_hip_set_sosfilt_tiled(ctx_, mode)); }
    // Welch power spectra of `rows` contiguous rows of x.size() / rows samples (kofft_hip_welch_f32): psd is resized to rows *
    // (win_len / 2 + 1) floats, (total * scale) (* 2 on the interior bins with `twice`) in the summation order the C header fixes
    // (groups of KOFFT_HIP_WELCH_GROUP frames).  window: win_len values, or empty for window::hann(win_len).  MismatchedLengths for rows
    // that do not divide x or a window of another size; then the C entry's checks in its order.  No detrending.
    Result welch(const std::vector<float> &x, const std::vector<float> &window, size_t win_len, size_t hop, size_t frames,
                 std::vector<float> &psd, size_t rows = 1, float scale = 1.0f, bool twice = false) const
    {
        static_assert(std::is_same<T, float>::value, "welch / csd are f32-only");
        if (rows == 0 || x.size() % rows != 0 || (!window.empty() && window.size() != win_len)) return Result::Err(FftError::MismatchedLengths);
        const size_t len = x.size() / rows;
        psd.assign(rows * (win_len / 2 + 1), 0.0f);
        return st(kofft_hip_welch_f32(ctx_, x.data(), rows, len, len, window.empty() ? nullptr : window.data(), win_len, hop, frames, scale,
                                      twice ? KOFFT_HIP_PSD_DOUBLE : 0, psd.data()));
    }
    // Cross spectra conj(X) Y of the rows of x and y (kofft_hip_csd_f32): pxy is resized to rows * (win_len / 2 + 1) complex values.
    Result csd(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &window, size_t win_len, size_t hop,
               size_t frames, std::vector<Complex<float>> &pxy, size_t rows = 1, float scale = 1.0f, bool twice = false) const
    {
        static_assert(std::is_same<T, float>::value, "welch / csd are f32-only");
        if (rows == 0 || x.size() % rows != 0 || y.size() != x.size() || (!window.empty() && window.size() != win_len))
            return Result::Err(FftError::MismatchedLengths);
        const size_t len = x.size() / rows;
        pxy.assign(rows * (win_len / 2 + 1), Complex<float>{0.0f, 0.0f});
        return st(kofft_hip_csd_f32(ctx_, x.data(), y.data(), rows, len, len, window.empty() ? nullptr : window.data(), win_len, hop, frames,
                                    scale, twice ? KOFFT_HIP_PSD_DOUBLE : 0, reinterpret_cast<float *>(pxy.data())));
    }
    // 1: the measured choice (the default), 0: every welch / csd of this context through the composed route, 2: the fused kernel
    // wherever it exists (the same bytes; A/B, tests)
    Result set_welch_fused(int mode) const { return st(kofft_hip_set_welch_fused(ctx_, mode)); }
    // kofft_hip_welch_scale_f32, no device: density 1 / (fs * sum w^2 * frames), spectrum 1 / ((sum w)^2 * frames); an empty window is
    // window::hann(win_len).  Returns 0 and sets `err` on an error (a zero sum, fs <= 0, frames == 0, win_len == 0).
    static float welch_scale(const std::vector<float> &window, size_t win_len, double fs, size_t frames, bool spectrum = false, int *err = nullptr)
    {
        float s = 0.0f;
        const int rc = (!window.empty() && window.size() != win_len)
                           ? KOFFT_ERR_MISMATCHED_LENGTHS
                           : kofft_hip_welch_scale_f32(window.empty() ? nullptr : window.data(), win_len, fs, frames, spectrum ? 1 : 0, &s);
        if (err) *err = rc;
        return rc ? 0.0f : s;
    }
    // cepstrum::mel_filterbank's sums (cepstrum.rs:51-67), f32 only like the reference: `rows` contiguous rows of mags.size() / rows
    // magnitudes in, rows of bins.size() - 2 energies out, with the filter edges `bins` (num_mel + 2 nondecreasing values; kofft::mel_bins
    // gives the reference-shaped ones).  MismatchedLengths for rows that do not divide the input, fewer than two edges or an output of
    // another size; InvalidValue for edges out of order; more than 4096 filters or rows over 2^24 throw DeviceError.
    Result mel_filterbank(const std::vector<float> &mags, const std::vector<uint64_t> &bins, std::vector<float> &energies, size_t rows = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the mel filterbank is f32-only (cepstrum.rs:36)");
        if (rows == 0 || mags.size() % rows != 0 || bins.size() < 2 || energies.size() != rows * (bins.size() - 2))
            return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_mel_filterbank_f32(ctx_, mags.data(), energies.data(), mags.size() / rows, rows, bins.data(), bins.size() - 2));
    }
    // cepstrum::mfcc / mfcc_batch (cepstrum.rs:72-98): the energies, logf(e + 1e-12f) with the libm crate's logf, the first num_coeffs
    // outputs of dct::dct2; coeffs: rows of num_coeffs.  InvalidValue for num_coeffs > bins.size() - 2 (cepstrum.rs:79), checked first
    // like the reference; otherwise as mel_filterbank.
    Result mfcc(const std::vector<float> &mags, const std::vector<uint64_t> &bins, size_t num_coeffs, std::vector<float> &coeffs, size_t rows = 1) const
    {
        static_assert(std::is_same<T, float>::value, "mfcc is f32-only (cepstrum.rs:72)");
        if (bins.size() >= 2 && num_coeffs > bins.size() - 2) return Result::Err(FftError::InvalidValue);
        if (rows == 0 || mags.size() % rows != 0 || bins.size() < 2 || coeffs.size() != rows * num_coeffs)
            return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_mfcc_f32(ctx_, mags.data(), coeffs.data(), mags.size() / rows, rows, bins.data(), bins.size() - 2, num_coeffs));
    }
    // ... on device memory, asynchronous on the context's stream (bins stays a host vector, read before the call returns); input and
    // output must not overlap (InvalidValue)
    Result mel_filterbank_dev(const float *d_mags, float *d_energies, size_t n_fft, size_t rows, const std::vector<uint64_t> &bins) const
    {
        static_assert(std::is_same<T, float>::value, "the mel filterbank is f32-only (cepstrum.rs:36)");
        if (bins.size() < 2) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_mel_filterbank_f32(ctx_, d_mags, d_energies, n_fft, rows, bins.data(), bins.size() - 2));
    }
    Result mfcc_dev(const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const std::vector<uint64_t> &bins, size_t num_coeffs) const
    {
        static_assert(std::is_same<T, float>::value, "mfcc is f32-only (cepstrum.rs:72)");
        if (bins.size() < 2) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_mfcc_f32(ctx_, d_mags, d_coeffs, n_fft, rows, bins.data(), bins.size() - 2, num_coeffs));
    }
    // 1 (the default): the fused kernel where it measured faster (up to 80 filters, 16 coefficients); 0: every MFCC composed; 2: fused wherever it fits (the same bytes)
    Result set_mfcc_fused(int mode) const { return st(kofft_hip_set_mfcc_fused(ctx_, mode)); }
    // The audio front end in one call (kofft_hip.h): stft_magnitudes -> mel_filterbank of `rows` signals of signals.size() / rows samples,
    // `frames` frames per row (0: ceil(len / hop)); energies: rows * frames * (bins.size() - 2), frame-major within a row, bit for bit what
    // stft_magnitudes_rows followed by mel_filterbank returns; the magnitudes stay on the device.  window empty: hann(win_len), else
    // win_len values.  InvalidHopSize first; MismatchedLengths for rows that do not divide the input, too few frames, a window of another
    // length, fewer than two edges or an output of another size; InvalidValue for edges out of order.
    Result stft_mel(const std::vector<float> &signals, size_t rows, size_t win_len, size_t hop, const std::vector<uint64_t> &bins,
                    std::vector<float> &energies, const std::vector<float> &window = {}, size_t frames = 0) const
    {
        static_assert(std::is_same<T, float>::value, "the audio front end is f32-only (cepstrum.rs:36)");
        if (hop == 0) return Result::Err(FftError::InvalidHopSize);
        if (rows == 0 || signals.size() % rows != 0 || bins.size() < 2 || (!window.empty() && window.size() != win_len))
            return Result::Err(FftError::MismatchedLengths);
        const size_t len = signals.size() / rows, need = len / hop + (len % hop != 0), nf = frames ? frames : need;
        if (energies.size() != rows * nf * (bins.size() - 2)) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_stft_mel_f32(ctx_, signals.data(), rows, len, len, window.empty() ? nullptr : window.data(), win_len, hop, nf, bins.data(),
                                         bins.size() - 2, energies.data()));
    }
    // ... through logf(e + 1e-12f) and the first num_coeffs outputs of dct::dct2: coeffs rows * frames * num_coeffs.  InvalidValue for
    // num_coeffs > bins.size() - 2 (cepstrum.rs:79); otherwise as stft_mel.
    Result stft_mfcc(const std::vector<float> &signals, size_t rows, size_t win_len, size_t hop, const std::vector<uint64_t> &bins, size_t num_coeffs,
                     std::vector<float> &coeffs, const std::vector<float> &window = {}, size_t frames = 0) const
    {
        static_assert(std::is_same<T, float>::value, "the audio front end is f32-only (cepstrum.rs:72)");
        if (hop == 0) return Result::Err(FftError::InvalidHopSize);
        if (bins.size() >= 2 && num_coeffs > bins.size() - 2) return Result::Err(FftError::InvalidValue);
        if (rows == 0 || signals.size() % rows != 0 || bins.size() < 2 || (!window.empty() && window.size() != win_len))
            return Result::Err(FftError::MismatchedLengths);
        const size_t len = signals.size() / rows, need = len / hop + (len % hop != 0), nf = frames ? frames : need;
        if (coeffs.size() != rows * nf * num_coeffs) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_stft_mfcc_f32(ctx_, signals.data(), rows, len, len, window.empty() ? nullptr : window.data(), win_len, hop, nf, bins.data(),
                                          bins.size() - 2, num_coeffs, coeffs.data()));
    }
    // ... on device memory, asynchronous on the context's stream: row r at d_signal + r * row_stride, d_window null for hann(win_len), bins a
    // host vector read before the call returns; the output must overlap neither the signal nor the window (InvalidValue)
    Result stft_mel_dev(const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len, size_t hop,
                        size_t frames, const std::vector<uint64_t> &bins, float *d_energies) const
    {
        static_assert(std::is_same<T, float>::value, "the audio front end is f32-only (cepstrum.rs:36)");
        if (bins.size() < 2) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_stft_mel_f32(ctx_, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins.data(), bins.size() - 2,
                                             d_energies));
    }
    Result stft_mfcc_dev(const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len, size_t hop,
                         size_t frames, const std::vector<uint64_t> &bins, size_t num_coeffs, float *d_coeffs) const
    {
        static_assert(std::is_same<T, float>::value, "the audio front end is f32-only (cepstrum.rs:72)");
        if (bins.size() < 2) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_stft_mfcc_f32(ctx_, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, bins.data(), bins.size() - 2,
                                              num_coeffs, d_coeffs));
    }
    // Audio -> spectrogram pictures in one call (kofft_hip.h): stft_magnitudes of `rows` signals of signals.size() / rows samples,
    // the maximum max_mode chooses (0: the row's, stft_magnitudes' own; 1: web-spectrogram's compute_frame's running maximum from 1e-12; 2:
    // max_in[r]) and spectrogram_render's colours, one dense picture per row: rows * frames * (win_len / 2) * channels Pixels, byte for byte
    // what stft_magnitudes_rows followed by spectrogram_render gives per row; the magnitudes stay on the device.  channels 4 (uint8_t only):
    // R, G, B, 255.  max_out receives the maximum used, one per row.  window empty: hann(win_len); frames 0: ceil(len / hop).
    // InvalidHopSize first; MismatchedLengths for rows that do not divide the input, too few frames, a window, a table, max_in or pictures
    // of another size; InvalidValue for the enums, channels 4 at 16 bits and max_mode 1 with scale 1.
    template <typename Pixel>
    Result stft_picture(const std::vector<float> &signals, size_t rows, size_t win_len, size_t hop, int max_mode, const std::vector<float> &max_in,
                        std::vector<float> &max_out, int mode, float level, int cmap, int channels, int scale, int layout,
                        const std::vector<uint32_t> &pix_of_bin, std::vector<Pixel> &out, const std::vector<float> &window = {},
                        size_t frames = 0) const
    {
        static_assert(std::is_same<T, float>::value, "the spectrogram pictures are f32-only (visual/spectrogram.rs)");
        static_assert(std::is_same<Pixel, uint8_t>::value || std::is_same<Pixel, uint16_t>::value, "pixels are uint8_t or uint16_t");
        if (hop == 0) return Result::Err(FftError::InvalidHopSize);
        if (rows == 0 || signals.size() % rows != 0 || (!window.empty() && window.size() != win_len)) return Result::Err(FftError::MismatchedLengths);
        const size_t len = signals.size() / rows, need = len / hop + (len % hop != 0), nf = frames ? frames : need;
        if (channels != 3 && channels != 4) return Result::Err(FftError::InvalidValue);
        if (out.size() != rows * nf * (win_len / 2) * (size_t)channels || (scale == 1 && pix_of_bin.size() != win_len / 2) ||
            (max_mode == 2 && max_in.size() != rows))
            return Result::Err(FftError::MismatchedLengths);
        max_out.assign(rows, 0.0f);
        return st(kofft_hip_stft_picture_f32(ctx_, signals.data(), rows, len, len, window.empty() ? nullptr : window.data(), win_len, hop, nf, max_mode,
                                             max_mode == 2 ? max_in.data() : nullptr, max_out.data(), mode, level, cmap, (int)(8 * sizeof(Pixel)),
                                             channels, scale, layout, scale == 1 ? pix_of_bin.data() : nullptr, out.data()));
    }
    // ... on device memory, asynchronous on the context's stream: d_window null for hann(win_len), d_max_in (max_mode 2) and d_max_out (null:
    // not wanted) device pointers to rows floats, pix_of_bin a host vector read before the call returns; d_out must overlap none of the others
    Result stft_picture_dev(const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len, size_t hop,
                            size_t frames, int max_mode, const float *d_max_in, float *d_max_out, int mode, float level, int cmap, int depth,
                            int channels, int scale, int layout, const std::vector<uint32_t> &pix_of_bin, void *d_out) const
    {
        static_assert(std::is_same<T, float>::value, "the spectrogram pictures are f32-only (visual/spectrogram.rs)");
        if (scale == 1 && pix_of_bin.size() != win_len / 2) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_stft_picture_f32(ctx_, d_signal, rows, len, row_stride, d_window, win_len, hop, frames, max_mode, d_max_in, d_max_out,
                                                 mode, level, cmap, depth, channels, scale, layout, scale == 1 ? pix_of_bin.data() : nullptr, d_out));
    }
    // 1 (the default): the measured choice (the composed route, which measured faster at every shape); 0: every call composed; 2:
    // the fused kernel wherever it fits (power-of-two windows of 64 .. 2048 samples, up to 128 filters) -- the same bytes
    Result set_frontend_fused(int mode) const { return st(kofft_hip_set_frontend_fused(ctx_, mode)); }
    // visual::spectrogram::magnitude_to_db / db_scale (spectrogram.rs:96-110) of every value, f32 only like the reference, with the libm
    // crate's log10f (kofft_hip.h: the arithmetic contract).  EmptyInput for no values, MismatchedLengths for an output of another size.
    Result magnitude_to_db(const std::vector<float> &mags, float max_mag, float floor_db, std::vector<float> &out) const
    {
        static_assert(std::is_same<T, float>::value, "the spectrogram helpers are f32-only (visual/spectrogram.rs)");
        if (out.size() != mags.size()) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_magnitude_to_db_f32(ctx_, mags.data(), mags.size(), &max_mag, floor_db, out.data()));
    }
    Result db_scale(const std::vector<float> &mags, float max_mag, float dynamic_range, std::vector<float> &out) const
    {
        static_assert(std::is_same<T, float>::value, "the spectrogram helpers are f32-only (visual/spectrogram.rs)");
        if (out.size() != mags.size()) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_db_scale_f32(ctx_, mags.data(), mags.size(), &max_mag, dynamic_range, out.data()));
    }
    // mags[frames][bins] -> an RGB picture of frames * bins * 3 values (kofft_hip.h: mode, level, cmap = KOFFT_CMAP_*, scale, layout);
    // Pixel = uint8_t (depth 8) or uint16_t (depth 16, the 8-bit value * 257).  pix_of_bin: the bins values of the log scale (kofft::log_bin_map
    // gives the reference-shaped ones), empty for the linear scale.  MismatchedLengths for frames that do not divide the input, a table
    // or an output of another size; InvalidValue for a colorous palette, an unknown enumerator or a table that decreases.
    template <typename Pixel>
    Result spectrogram_render(const std::vector<float> &mags, size_t frames, float max_mag, int mode, float level, int cmap, int scale, int layout,
                              const std::vector<uint32_t> &pix_of_bin, std::vector<Pixel> &out) const
    {
        static_assert(std::is_same<T, float>::value, "the spectrogram helpers are f32-only (visual/spectrogram.rs)");
        static_assert(std::is_same<Pixel, uint8_t>::value || std::is_same<Pixel, uint16_t>::value, "pixels are uint8_t or uint16_t");
        if (frames == 0 || mags.empty()) return Result::Err(FftError::EmptyInput);
        if (mags.size() % frames != 0 || out.size() != mags.size() * 3 || (scale == 1 && pix_of_bin.size() != mags.size() / frames))
            return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_spectrogram_render_f32(ctx_, mags.data(), frames, mags.size() / frames, &max_mag, mode, level, cmap, (int)(8 * sizeof(Pixel)),
                                                   scale, layout, scale == 1 ? pix_of_bin.data() : nullptr, out.data()));
    }
    // ... on device memory, asynchronous on the context's stream: d_max_mag is a device pointer (the d_max of stft_magnitudes), pix_of_bin
    // stays a host vector, read before the call returns; the output must not overlap the input or d_max_mag (InvalidValue)
    Result magnitude_to_db_dev(const float *d_mags, size_t count, const float *d_max_mag, float floor_db, float *d_out) const
    {
        return st(kofft_hip_dev_magnitude_to_db_f32(ctx_, d_mags, count, d_max_mag, floor_db, d_out));
    }
    Result db_scale_dev(const float *d_mags, size_t count, const float *d_max_mag, float dynamic_range, float *d_out) const
    {
        return st(kofft_hip_dev_db_scale_f32(ctx_, d_mags, count, d_max_mag, dynamic_range, d_out));
    }
    Result spectrogram_render_dev(const float *d_mags, size_t frames, size_t bins, const float *d_max_mag, int mode, float level, int cmap, int depth,
                                  int scale, int layout, const std::vector<uint32_t> &pix_of_bin, void *d_out) const
    {
        if (scale == 1 && pix_of_bin.size() != bins) return Result::Err(FftError::MismatchedLengths);
        return st(kofft_hip_dev_spectrogram_render_f32(ctx_, d_mags, frames, bins, d_max_mag, mode, level, cmap, depth, scale, layout,
                                                       scale == 1 ? pix_of_bin.data() : nullptr, d_out));
    }
    // true (the default): the image layout leaves through an LDS tile, whole dwords per picture row; false: every lane stores its own bytes (the same bytes)
    Result set_spectrogram_transpose(bool on) const { return st(kofft_hip_set_spectrogram_transpose(ctx_, on ? 1 : 0)); }
    // dct::dct1 .. dct4 (dct.rs:108-176; type 1 .. 4), the direct sums, f32 only like the reference: `batch` contiguous rows of n reals
    // in, rows of n reals out.  MismatchedLengths for rows that do not divide the input or an output of another size; InvalidValue for
    // a type outside 1 .. 4; n == 0 is an empty result except for type 3 (EmptyInput: dct3 indexes input[0] unchecked); n > 4096
    // throws DeviceError (the table bound).  input and output may be the same vector.  Type 2 is dct::dct2, not plan_dct2 (dct2).
    Result dct_direct(int type, const std::vector<float> &input, std::vector<float> &output, size_t batch = 1) const
    {
        return direct(kofft_hip_dct_direct_f32, type, input, output, batch);
    }
    // dst::dst1 .. dst4 (dst.rs:89-146; type 1 .. 4): as dct_direct (dst3: EmptyInput at n == 0).
    Result dst_direct(int type, const std::vector<float> &input, std::vector<float> &output, size_t batch = 1) const
    {
        return direct(kofft_hip_dst_direct_f32, type, input, output, batch);
    }

    Result direct(int (*fn)(kofft_hip_ctx *, int, const float *, float *, size_t, size_t), int type, const std::vector<float> &input,
                  std::vector<float> &output, size_t batch) const
    {
        static_assert(std::is_same<T, float>::value, "the direct DCT / DST are f32-only (dct.rs / dst.rs)");
        if (type < 1 || type > 4) return Result::Err(FftError::InvalidValue);
        if (batch == 0 || input.size() % batch != 0 || output.size() != input.size()) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        if (n == 0) return type == 3 ? Result::Err(FftError::EmptyInput) : Result::Ok();
        return st(fn(ctx_, type, input.data(), output.data(), n, batch));
    }

    // hartley::dht (hartley.rs:12-27) on batch rows of input.size() / batch reals, bit for bit the reference's sums with the libm
    // crate's cosf / sinf.  MismatchedLengths for rows that do not divide the input or an output of another size; n == 0 is an empty
    // result; n > 4096 throws DeviceError (the table bound).  input and output may be the same vector (hartley::batch is in place).
    Result dht(const std::vector<float> &input, std::vector<float> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the Hartley transform is f32-only (hartley.rs)");
        if (batch == 0 || input.size() % batch != 0 || output.size() != input.size()) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        if (n == 0) return Result::Ok();
        return st(kofft_hip_dht_f32(ctx_, input.data(), output.data(), n, batch));
    }
    // ... on device memory, asynchronous on the context's stream; the two must not overlap (InvalidValue)
    Result dht_dev(const float *d_in, float *d_out, size_t n, size_t batch) const
    {
        static_assert(std::is_same<T, float>::value, "the Hartley transform is f32-only (hartley.rs)");
        return st(kofft_hip_dev_dht_f32(ctx_, d_in, d_out, n, batch));
    }
    // true (the default): the table of a new length is built by a kernel; false: on the host and uploaded (the same bytes)
    Result set_dht_table_device(bool on) const { return st(kofft_hip_set_dht_table_device(ctx_, on ? 1 : 0)); }

    // wavelet::<name>_forward (wavelet.rs:12-21, 154-493; wavelet = KOFFT_WAVELET_HAAR .. COIF1), f32 only like the reference: `batch`
    // contiguous rows of len samples in; approx and detail become batch rows of len / 2.  InvalidValue for an unknown wavelet;
    // MismatchedLengths for rows that do not divide the input; rows over 2^26 throw DeviceError.
    Result dwt(int wavelet, const std::vector<float> &input, std::vector<float> &approx, std::vector<float> &detail, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the wavelet transforms are f32-only (wavelet.rs)");
        if (wavelet < 0 || wavelet > 4) return Result::Err(FftError::InvalidValue);
        if (batch == 0 || input.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t len = input.size() / batch;
        approx.assign(batch * (len / 2), 0.0f);
        detail.assign(batch * (len / 2), 0.0f);
        if (len / 2 == 0) return Result::Ok();
        return st(kofft_hip_dwt_f32(ctx_, wavelet, input.data(), approx.data(), detail.data(), len, batch));
    }
    // wavelet::<name>_inverse (wavelet.rs:24-33, 190-535): batch rows of n approximations and batch rows of at least n details (the
    // entries past n are ignored, as in the reference); output becomes batch rows of 2n.  MismatchedLengths for rows that do not
    // divide the inputs or details shorter than the approximations (the reference panics there).
    Result idwt(int wavelet, const std::vector<float> &approx, const std::vector<float> &detail, std::vector<float> &output,
                size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the wavelet transforms are f32-only (wavelet.rs)");
        if (wavelet < 0 || wavelet > 4) return Result::Err(FftError::InvalidValue);
        if (batch == 0 || approx.size() % batch != 0 || detail.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t n = approx.size() / batch, dn = detail.size() / batch;
        if (dn < n) return Result::Err(FftError::MismatchedLengths);
        output.assign(2 * approx.size(), 0.0f);
        if (n == 0) return Result::Ok();
        if (dn == n) return st(kofft_hip_idwt_f32(ctx_, wavelet, approx.data(), detail.data(), output.data(), n, batch));
        return st(kofft_hip_idwt_multi_f32(ctx_, wavelet, approx.data(), detail.data(), &dn, output.data(), n, batch, 1));  // (detail stride dn)
    }
    // wavelet::multi_level_forward with <name>_forward (wavelet.rs:54-71, 538-566): approx becomes batch rows of a_L, details[l]
    // (finest first) batch rows of a_l, a_l = ceil(a_{l-1} / 2) (an odd row is padded with its last sample before each level).
    Result dwt_multi(int wavelet, const std::vector<float> &input, size_t levels, std::vector<float> &approx,
                     std::vector<std::vector<float>> &details, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the wavelet transforms are f32-only (wavelet.rs)");
        if (wavelet < 0 || wavelet > 4) return Result::Err(FftError::InvalidValue);
        if (batch == 0 || input.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t len = input.size() / batch;
        if (levels > 64 || len > (size_t(1) << 26)) return st(KOFFT_ERR_UNSUPPORTED);  // (before anything is allocated)
        std::vector<size_t> lens(levels + 1);
        const int lrc = kofft_hip_dwt_multi_lengths(len, levels, lens.data());
        if (lrc) return st(lrc);
        size_t total = 0;
        for (size_t l = 1; l <= levels; ++l) total += lens[l];
        approx.assign(batch * lens[levels], 0.0f);
        std::vector<float> packed(batch * total);
        details.assign(levels, {});
        if (len != 0) {
            const Result r = st(kofft_hip_dwt_multi_f32(ctx_, wavelet, input.data(), approx.data(), packed.data(), len, batch, levels));
            if (r.is_err()) return r;
        }
        size_t off = 0;
        for (size_t l = 1; l <= levels; ++l) {
            details[l - 1].assign(packed.begin() + off, packed.begin() + off + batch * lens[l]);
            off += batch * lens[l];
        }
        return Result::Ok();
    }
    // wavelet::multi_level_inverse with <name>_inverse (wavelet.rs:74-84, 538-566): batch rows of n approximations, details[l] batch
    // rows each (finest first); output becomes batch rows of n << levels.  MismatchedLengths where the reference would index past a
    // detail (it panics there) or for rows that do not divide the inputs.
    Result idwt_multi(int wavelet, const std::vector<float> &approx, const std::vector<std::vector<float>> &details,
                      std::vector<float> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the wavelet transforms are f32-only (wavelet.rs)");
        if (wavelet < 0 || wavelet > 4) return Result::Err(FftError::InvalidValue);
        if (batch == 0 || approx.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t n = approx.size() / batch, levels = details.size();
        std::vector<size_t> lens(levels ? levels : 1);
        std::vector<float> packed;
        for (size_t l = 0; l < levels; ++l) {
            if (details[l].size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
            lens[l] = details[l].size() / batch;
            packed.insert(packed.end(), details[l].begin(), details[l].end());
        }
        if (n == 0) {
            output.clear();
            return Result::Ok();
        }
        // the output is allocated only for lengths the C ABI takes; otherwise it returns MismatchedLengths or UNSUPPORTED before it
        // looks at the (null) output
        const bool fits = levels <= 64 && n <= (size_t(1) << 26) && (n << levels) <= (size_t(1) << 26);
        float *dst = nullptr;
        if (fits) {
            output.assign(batch * (n << levels), 0.0f);
            dst = output.data();
        }
        const float *pd = packed.empty() ? approx.data() : packed.data();
        return st(kofft_hip_idwt_multi_f32(ctx_, wavelet, approx.data(), pd, lens.data(), dst, n, batch, levels));
    }

    // czt::czt_f32 (czt.rs:16-54): batch rows of input.size() / batch reals; output becomes batch rows of m complex bins.  m == 0 gives
    // an empty output, an empty row m bins of (+0, +0), as in the reference.  MismatchedLengths for rows that do not divide the input.
    Result czt(const std::vector<float> &input, size_t m, Complex32 w, Complex32 a, std::vector<Complex32> &output, size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the chirp-Z transform is f32-only (czt.rs)");
        if (batch == 0 || input.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        const bool fits = n <= 4096 && m <= 4096;  // beyond: the C ABI returns UNSUPPORTED before it looks at the output
        output.assign(fits ? batch * m : 0, Complex32::zero());
        if (m == 0) return Result::Ok();
        return st(kofft_hip_czt_f32(ctx_, input.data(), reinterpret_cast<float *>(output.data()), n, m, w.re, w.im, a.re, a.im, batch));
    }
    // ... on device memory, asynchronous on the context's stream: batch rows of n floats in, batch rows of m complex out; the two must
    // not overlap (InvalidValue)
    Result czt_dev(const float *d_in, float *d_out, size_t n, size_t m, Complex32 w, Complex32 a, size_t batch) const
    {
        static_assert(std::is_same<T, float>::value, "the chirp-Z transform is f32-only (czt.rs)");
        return st(kofft_hip_dev_czt_f32(ctx_, d_in, d_out, n, m, w.re, w.im, a.re, a.im, batch));
    }
    // 0: by batch and by whether the table is already there; 1 / 2: always sums on the fly / always a device-built table (the same bytes)
    Result set_czt_route(int mode) const { return st(kofft_hip_set_czt_route(ctx_, mode)); }
    // goertzel::goertzel_f32 (goertzel.rs:16-36) of batch rows against every one of target_freqs: output becomes batch rows of
    // target_freqs.size() magnitudes.  EmptyInput for empty rows, then InvalidValue for sample_rate <= 0, as in the reference.
    Result goertzel(const std::vector<float> &input, float sample_rate, const std::vector<float> &target_freqs, std::vector<float> &output,
                    size_t batch = 1) const
    {
        static_assert(std::is_same<T, float>::value, "the Goertzel detector is f32-only (goertzel.rs)");
        if (batch == 0 || input.size() % batch != 0) return Result::Err(FftError::MismatchedLengths);
        const size_t n = input.size() / batch;
        const bool fits = n <= (size_t(1) << 26) && target_freqs.size() <= 1024;
        output.assign(fits ? batch * target_freqs.size() : 0, 0.0f);
        return st(kofft_hip_goertzel_f32(ctx_, input.data(), output.data(), n, batch, sample_rate, target_freqs.data(), target_freqs.size()));
    }
    // the reference's call: one row, one frequency
    Result goertzel(const std::vector<float> &input, float sample_rate, float target_freq, float &magnitude) const
    {
        std::vector<float> out;
        Result r = goertzel(input, sample_rate, std::vector<float>{target_freq}, out);
        if (r.is_ok()) magnitude = out[0];
        return r;
    }
    // ... on device memory (target_freqs stays a host array), asynchronous on the context's stream
    Result goertzel_dev(const float *d_in, float *d_out, size_t n, size_t batch, float sample_rate, const std::vector<float> &target_freqs) const
    {
        static_assert(std::is_same<T, float>::value, "the Goertzel detector is f32-only (goertzel.rs)");
        return st(kofft_hip_dev_goertzel_f32(ctx_, d_in, d_out, n, batch, sample_rate, target_freqs.data(), target_freqs.size()));
    }

    // added: contiguous batch (fft::batch over one buffer)
    Result fft_batch(std::vector<C> &data, size_t n, bool inverse = false) const
    {
        if (n != 0 && data.size() % n != 0) return Result::Err(FftError::MismatchedLengths);
        return st(detail::Abi<T>::fft(ctx_, fp(data), n, n ? data.size() / n : 1, inverse ? 1 : 0));
    }

    Result st(int rc) const
    {
        if (rc == 0) return Result::Ok();
        if (rc > 0) return Result::Err(static_cast<FftError>(rc));
        throw DeviceError(rc, kofft_hip_last_error(ctx_));
    }

private:
    static T *fp(std::vector<C> &v) { return reinterpret_cast<T *>(v.data()); }
    Result convolve_impl(const std::vector<float> &x, const std::vector<float> &h, size_t nh, std::vector<float> &out, size_t rows,
                         size_t block, size_t first, size_t count, unsigned flags) const
    {
        static_assert(std::is_same<T, float>::value, "convolve_rows / correlate_rows are f32-only");
        if (rows == 0 || x.size() % rows != 0 || (h.size() != nh && h.size() != rows * nh)) return Result::Err(FftError::MismatchedLengths);
        const size_t nx = x.size() / rows;
        if (nx == 0 || nh == 0) return Result::Err(FftError::EmptyInput);
        const size_t full = nx + nh - 1;
        if (count == SIZE_MAX) {
            if (first > full) return Result::Err(FftError::MismatchedLengths);
            count = full - first;
        }
        if (first > full || count > full - first) return Result::Err(FftError::MismatchedLengths);
        out.resize(rows * count);
        float dummy = 0.0f;  // (count == 0: the C entry returns before it looks at the pointer)
        return st(kofft_hip_convolve_f32(ctx_, x.data(), rows, nx, h.data(), h.size() == nh ? 1 : rows, nh, block, flags,
                                         out.empty() ? &dummy : out.data(), first, count));
    }
    Result oop_strided(const std::vector<C> &input, size_t in_stride, std::vector<C> &output, size_t out_stride,
                       bool inverse) const  // fft.rs:1261-1336
    {
        if (in_stride == 0 || out_stride == 0) return Result::Err(FftError::InvalidStride);
        if (input.size() % in_stride != 0 || output.size() % out_stride != 0) return Result::Err(FftError::InvalidStride);
        const size_t n = input.size() / in_stride;
        if (output.size() / out_stride != n) return Result::Err(FftError::MismatchedLengths);
        std::vector<C> scratch(n);
        for (size_t i = 0; i < n; ++i) scratch[i] = input[i * in_stride];
        Result r = inverse ? ifft(scratch) : fft(scratch);
        if (r.is_err()) return r;
        for (size_t i = 0; i < n; ++i) output[i * out_stride] = scratch[i];
        return Result::Ok();
    }
    kofft_hip_ctx *ctx_ = nullptr;
};

template <typename T>
class FftPlanner {  // fft.rs:332-445
public:
    std::vector<Complex<T>> get_twiddles(size_t n) const
    {
        std::vector<Complex<T>> t(n / 2);
        detail::Abi<T>::twiddles(n, reinterpret_cast<T *>(t.data()));
        return t;
    }
    FftStrategy plan_strategy(size_t n) const { return (n > 1 && (n & (n - 1)) == 0) ? FftStrategy::SplitRadix : FftStrategy::Auto; }
};

template <typename T>
class RfftPlanner {  // rfft.rs:194-338
public:
    std::vector<Complex<T>> get_twiddles(size_t m) const
    {
        std::vector<Complex<T>> t(m);
        detail::Abi<T>::rfft_table(m, reinterpret_cast<T *>(t.data()));
        return t;
    }
    Result rfft_with_scratch(const HipFftImpl<T> &fft, std::vector<T> &input, std::vector<Complex<T>> &output,
                             std::vector<Complex<T>> &scratch) const
    {
        return fft.rfft_with_scratch(input, output, scratch);
    }
    Result irfft_with_scratch(const HipFftImpl<T> &fft, std::vector<Complex<T>> &input, std::vector<T> &output,
                              std::vector<Complex<T>> &scratch) const
    {
        return fft.irfft_with_scratch(input, output, scratch);
    }
};

// num.rs:236-261: a view of two caller-owned planes.  The constructor does not compare the lengths (the reference's struct literal does
// not either, tests/split.rs:65-74: fft_split_complex then returns MismatchedLengths); new_() asserts like SplitComplex::new.
template <typename T>
struct SplitComplex {
    std::vector<T> &re, &im;
    SplitComplex(std::vector<T> &r, std::vector<T> &i) : re(r), im(i) {}
    static SplitComplex new_(std::vector<T> &r, std::vector<T> &i)
    {
        if (r.size() != i.size()) throw std::logic_error("SplitComplex::new: re.len() != im.len()");
        return SplitComplex(r, i);
    }
    size_t len() const { return re.size(); }
    bool is_empty() const { return re.empty(); }
    static SplitComplex copy_from_complex(const std::vector<Complex<T>> &input, std::vector<T> &r, std::vector<T> &i)  // num.rs:332-339
    {
        if (input.size() != r.size() || input.size() != i.size()) throw std::logic_error("copy_from_complex: lengths differ");
        for (size_t k = 0; k < input.size(); ++k) { r[k] = input[k].re; i[k] = input[k].im; }
        return SplitComplex(r, i);
    }
    void copy_to_complex(std::vector<Complex<T>> &out) const  // num.rs:341-348
    {
        if (re.size() != im.size() || re.size() != out.size()) throw std::logic_error("copy_to_complex: lengths differ");
        for (size_t k = 0; k < re.size(); ++k) out[k] = Complex<T>(re[k], im[k]);
    }
};
using SplitComplex32 = SplitComplex<float>;
using SplitComplex64 = SplitComplex<double>;

// num.rs:264-308: two owned f32 planes
struct ComplexVec {
    std::vector<float> re, im;
    ComplexVec() = default;
    ComplexVec(std::vector<float> r, std::vector<float> i) : re(std::move(r)), im(std::move(i))
    {
        if (re.size() != im.size()) throw std::logic_error("ComplexVec::new: re.len() != im.len()");
    }
    size_t len() const { return re.size(); }
    bool is_empty() const { return re.empty(); }
    static ComplexVec from_complex_vec(const std::vector<Complex32> &v)
    {
        ComplexVec c;
        c.re.reserve(v.size());
        c.im.reserve(v.size());
        for (const Complex32 &x : v) { c.re.push_back(x.re); c.im.push_back(x.im); }
        return c;
    }
    std::vector<Complex32> to_complex_vec() const
    {
        std::vector<Complex32> out(re.size());
        for (size_t k = 0; k < re.size(); ++k) out[k] = Complex32(re[k], im[k]);
        return out;
    }
    bool operator==(const ComplexVec &o) const { return re == o.re && im == o.im; }
};

// fft::fft_split / ifft_split / fft_split_complex / ifft_split_complex / fft_complex_vec / ifft_complex_vec (fft.rs:2129-2153).  The
// reference builds ScalarFftImpl::default() per call; here the caller passes the implementation, as for batch() below.
template <typename T>
Result fft_split(const FftImpl<T> &fft, std::vector<T> &re, std::vector<T> &im) { return fft.fft_split(re, im); }
template <typename T>
Result ifft_split(const FftImpl<T> &fft, std::vector<T> &re, std::vector<T> &im) { return fft.ifft_split(re, im); }
template <typename T>
Result fft_split_complex(const FftImpl<T> &fft, SplitComplex<T> data) { return fft.fft_split(data.re, data.im); }
template <typename T>
Result ifft_split_complex(const FftImpl<T> &fft, SplitComplex<T> data) { return fft.ifft_split(data.re, data.im); }
inline Result fft_complex_vec(const FftImpl<float> &fft, ComplexVec &data) { return fft.fft_split(data.re, data.im); }
inline Result ifft_complex_vec(const FftImpl<float> &fft, ComplexVec &data) { return fft.ifft_split(data.re, data.im); }

// fft::FftPlan (fft.rs:1989-2094): a length and a strategy bound to an implementation.  FftPlan::fft (fft.rs:2012-2038):
// an f32 plan with strategy Radix2 / Radix4 takes the *_with_twiddles shortcut, and every *_with_twiddles is stockham_fft
// (fft.rs:1645-1660) -- the Stockham transform, NOT fft_radix4; every other plan goes through fft_with_strategy, where
// Radix4 means fft_radix4.  FftPlan::ifft (fft.rs:2040-2055) = conj, that same fft, conj * 1/(n as f32).  Not reproduced:
// the reference's f32 Radix2 / Radix4 plan of length 1 panics (unreachable!() in stockham_fft, fft.rs:655-662); identity here.
template <typename T>
class FftPlan {
public:
    size_t n;
    FftStrategy strategy;
    FftPlan(size_t n_, FftStrategy s, const HipFftImpl<T> &f) : n(n_), strategy(s), fft_(f) {}
    Result fft(std::vector<Complex<T>> &input) const
    {
        if (input.size() != n) return Result::Err(FftError::MismatchedLengths);
        if (stockham_shortcut()) return n == 1 ? Result::Ok() : fft_.fft(input);
        return fft_.fft_with_strategy(input, strategy);
    }
    Result ifft(std::vector<Complex<T>> &input) const
    {
        if (input.size() != n) return Result::Err(FftError::MismatchedLengths);
        if (n <= 1) return fft(input);
        if (strategy == FftStrategy::Radix4 && fft_.radix4_compat && !stockham_shortcut()) return fft_.ifft_radix4(input);
        return fft_.ifft(input);  // conj, fft, conj, * 1/(n as f32): ifft's arithmetic
    }
    Result fft_out_of_place(const std::vector<Complex<T>> &input, std::vector<Complex<T>> &output) const
    {
        if (input.size() != n || output.size() != n) return Result::Err(FftError::MismatchedLengths);
        output = input;
        return fft(output);
    }
    Result ifft_out_of_place(const std::vector<Complex<T>> &input, std::vector<Complex<T>> &output) const
    {
        if (input.size() != n || output.size() != n) return Result::Err(FftError::MismatchedLengths);
        output = input;
        return ifft(output);
    }
    Result fft_split(std::vector<T> &re, std::vector<T> &im) const  // fft.rs:2081-2086
    {
        if (re.size() != n || im.size() != n) return Result::Err(FftError::MismatchedLengths);
        return fft_.fft_split(re, im);
    }
    Result ifft_split(std::vector<T> &re, std::vector<T> &im) const  // fft.rs:2088-2093
    {
        if (re.size() != n || im.size() != n) return Result::Err(FftError::MismatchedLengths);
        return fft_.ifft_split(re, im);
    }
    // fft.rs:2096-2112 (FftPlan<f32> in the reference)
    template <typename U = T, typename = std::enable_if_t<std::is_same<U, float>::value>>
    Result fft_complex_vec(ComplexVec &data) const
    {
        if (data.len() != n) return Result::Err(FftError::MismatchedLengths);
        return fft_.fft_split(data.re, data.im);
    }
    template <typename U = T, typename = std::enable_if_t<std::is_same<U, float>::value>>
    Result ifft_complex_vec(ComplexVec &data) const
    {
        if (data.len() != n) return Result::Err(FftError::MismatchedLengths);
        return fft_.ifft_split(data.re, data.im);
    }

private:
    bool stockham_shortcut() const  // fft.rs:2016-2035
    {
        return sizeof(T) == 4 && (strategy == FftStrategy::Radix2 || strategy == FftStrategy::Radix4);
    }
    const HipFftImpl<T> &fft_;
};

// rfft::rfft_packed / irfft_packed (rfft.rs:341-420): the same checks and arithmetic as rfft_direct / irfft_direct
template <typename T>
Result rfft_packed(RfftPlanner<T> &, const HipFftImpl<T> &fft, std::vector<T> &input, std::vector<Complex<T>> &output,
                   std::vector<Complex<T>> &scratch)
{
    return fft.rfft_with_scratch(input, output, scratch);
}
template <typename T>
Result irfft_packed(RfftPlanner<T> &, const HipFftImpl<T> &fft, std::vector<Complex<T>> &input, std::vector<T> &output,
                    std::vector<Complex<T>> &scratch)
{
    return fft.irfft_with_scratch(input, output, scratch);
}

// fft::batch / batch_inverse / multi_channel (fft.rs:2156-2191): serial semantics, first error wins
template <typename T>
Result batch(const FftImpl<T> &fft, std::vector<std::vector<Complex<T>>> &batches)
{
    for (auto &b : batches) {
        Result r = fft.fft(b);
        if (r.is_err()) return r;
    }
    return Result::Ok();
}
template <typename T>
Result batch_inverse(const FftImpl<T> &fft, std::vector<std::vector<Complex<T>>> &batches)
{
    for (auto &b : batches) {
        Result r = fft.ifft(b);
        if (r.is_err()) return r;
    }
    return Result::Ok();
}
template <typename T>
Result multi_channel(const FftImpl<T> &fft, std::vector<std::vector<Complex<T>>> &channels) { return batch(fft, channels); }

inline std::vector<float> hann(size_t len)  // window.rs:24-28
{
    std::vector<float> w(len);
    kofft_hip_hann_f32(len, w.data());
    return w;
}
// window::hamming / blackman / kaiser (window.rs:31-61), window_more::tukey / bartlett / bohman / nuttall (window_more.rs:13-64):
// kind = KOFFT_WINDOW_*, param = kaiser's beta or tukey's alpha.  An unknown kind and kaiser of length 0 (the reference underflows
// `len - 1` there) throw std::invalid_argument.
inline std::vector<float> window(int kind, size_t len, float param = 0.0f)
{
    std::vector<float> w(len);
    if (kofft_hip_window_f32(kind, len, param, w.data()) != 0) throw std::invalid_argument("kofft::window: unknown kind, or kaiser of length 0");
    return w;
}
inline std::vector<float> hamming(size_t len) { return window(KOFFT_WINDOW_HAMMING, len); }
inline std::vector<float> blackman(size_t len) { return window(KOFFT_WINDOW_BLACKMAN, len); }
inline std::vector<float> kaiser(size_t len, float beta) { return window(KOFFT_WINDOW_KAISER, len, beta); }
inline std::vector<float> tukey(size_t len, float alpha) { return window(KOFFT_WINDOW_TUKEY, len, alpha); }
inline std::vector<float> bartlett(size_t len) { return window(KOFFT_WINDOW_BARTLETT, len); }
inline std::vector<float> bohman(size_t len) { return window(KOFFT_WINDOW_BOHMAN, len); }
inline std::vector<float> nuttall(size_t len) { return window(KOFFT_WINDOW_NUTTALL, len); }
// The filter edges of cepstrum::mel_filterbank (cepstrum.rs:38-50) for rows of n_fft magnitudes: num_filters + 2 values, f32 in the
// reference's order with GLIBC's log10f / powf where the reference calls the libm crate's -- equal to the crate's wherever the exact
// edge is not within an ulp of an integer; the last edge of an odd n_fft is the known case that is not pinned (kofft_hip.h).  More
// than 4096 filters throw std::invalid_argument.
inline std::vector<uint64_t> mel_bins(float sample_rate, size_t n_fft, size_t num_filters)
{
    std::vector<uint64_t> bins(num_filters + 2);
    if (kofft_hip_mel_bins_f32(sample_rate, n_fft, num_filters, bins.data()) != 0) throw std::invalid_argument("kofft::mel_bins: more than 4096 filters");
    return bins;
}

// visual::spectrogram::map_bin_to_pixel(b, bins - 1) for every b < bins (spectrogram.rs:209-217), f32 with GLIBC's logf: the table the
// log-scaled render takes.  bins == 0 or > 2^24 throw std::invalid_argument.
inline std::vector<uint32_t> log_bin_map(size_t bins)
{
    std::vector<uint32_t> table(bins);
    if (kofft_hip_log_bin_map(bins, table.data()) != 0) throw std::invalid_argument("kofft::log_bin_map: bins must be 1 .. 2^24");
    return table;
}
// visual::spectrogram::map_color_u8 (spectrogram.rs:113-160) on the host; a colorous palette or an unknown cmap throws std::invalid_argument.
inline std::array<uint8_t, 3> map_color_u8(float t, int cmap)
{
    std::array<uint8_t, 3> rgb{};
    if (kofft_hip_map_color_u8(t, cmap, rgb.data()) != 0) throw std::invalid_argument("kofft::map_color_u8: Fire, Legacy, Gray and Rainbow are implemented");
    return rgb;
}

// stft::stft (stft.rs:76-105): output frames are resized to the window length and overwritten
inline Result stft(const std::vector<float> &signal, const std::vector<float> &window, size_t hop_size,
                   std::vector<std::vector<Complex32>> &output, const HipFftImpl<float> &fft, bool check_frames = true)
{
    const size_t frames = output.size(), wl = window.size();
    std::vector<Complex32> flat(frames * wl);
    int rc = check_frames
                 ? kofft_hip_stft_f32(fft.raw(), signal.data(), signal.size(), window.data(), wl, hop_size,
                                      reinterpret_cast<float *>(flat.data()), frames)
                 : kofft_hip_stft_parallel_f32(fft.raw(), signal.data(), signal.size(), window.data(), wl, hop_size,
                                               reinterpret_cast<float *>(flat.data()), frames);
    Result r = fft.st(rc);
    if (r.is_err()) return r;
    for (size_t f = 0; f < frames; ++f) output[f].assign(flat.begin() + f * wl, flat.begin() + (f + 1) * wl);
    return Result::Ok();
}
// stft::istft (stft.rs:117-156): frames are inverse-transformed in place; output is accumulated into and normalised
inline Result istft(std::vector<std::vector<Complex32>> &frames, const std::vector<float> &window, size_t hop_size,
                    std::vector<float> &output, std::vector<float> &scratch, const HipFftImpl<float> &fft)
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);
    if (scratch.size() != output.size()) return Result::Err(FftError::MismatchedLengths);
    const size_t wl = window.size();
    for (auto &f : frames)
        if (f.size() != wl) return Result::Err(FftError::MismatchedLengths);
    std::vector<Complex32> flat(frames.size() * wl);
    for (size_t f = 0; f < frames.size(); ++f) std::copy(frames[f].begin(), frames[f].end(), flat.begin() + f * wl);
    Result r = fft.st(kofft_hip_istft_f32(fft.raw(), reinterpret_cast<float *>(flat.data()), frames.size(), window.data(), wl,
                                          hop_size, output.data(), output.size(), scratch.data(), scratch.size()));
    if (r.is_err()) return r;
    for (size_t f = 0; f < frames.size(); ++f) frames[f].assign(flat.begin() + f * wl, flat.begin() + (f + 1) * wl);
    return Result::Ok();
}
// stft::inverse_parallel (stft.rs:289-343): frames are left untouched, samples whose window-square sum is <= 1e-8
// become 0; only hop == 0 is rejected (a frame shorter than the window panics in the reference: out_of_range here)
inline Result inverse_parallel(const std::vector<std::vector<Complex32>> &frames, const std::vector<float> &window,
                               size_t hop_size, std::vector<float> &output, const HipFftImpl<float> &fft)
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);
    const size_t wl = window.size();
    std::vector<Complex32> flat(frames.size() * wl);
    for (size_t f = 0; f < frames.size(); ++f) {
        if (frames[f].size() != wl) throw std::out_of_range("frame length differs from the window (the reference panics)");
        std::copy(frames[f].begin(), frames[f].end(), flat.begin() + f * wl);
    }
    return fft.st(kofft_hip_istft_parallel_f32(fft.raw(), reinterpret_cast<const float *>(flat.data()), frames.size(),
                                               window.data(), wl, hop_size, output.data(), output.size()));
}
// stft::inverse_frame (stft.rs:384-399): ifft(frame) in place, windowed add into output from `start`, no normalisation
inline Result inverse_frame(std::vector<Complex32> &frame_io, const std::vector<float> &window, size_t start,
                            std::vector<float> &output, const HipFftImpl<float> &fft)
{
    if (frame_io.size() != window.size()) throw std::out_of_range("frame length differs from the window (the reference panics)");
    return fft.st(kofft_hip_istft_frame_f32(fft.raw(), reinterpret_cast<float *>(frame_io.data()), window.data(), window.size(),
                                            start, output.data(), output.size()));
}
// visual::spectrogram::stft_magnitudes (visual/spectrogram.rs:52-76): (frames x win_len/2 magnitudes, max magnitude)
inline Result stft_magnitudes(const std::vector<float> &samples, size_t win_len, size_t hop,
                              std::vector<std::vector<float>> &mags, float &max_mag, const HipFftImpl<float> &fft)
{
    if (hop == 0) return Result::Err(FftError::InvalidHopSize);  // the reference divides by hop (panic)
    const size_t frames = (samples.size() + hop - 1) / hop, half = win_len / 2;
    std::vector<float> flat(frames * half);
    Result r = fft.st(kofft_hip_stft_magnitudes_f32(fft.raw(), samples.data(), samples.size(), win_len, hop, flat.data(), frames,
                                                    &max_mag));
    if (r.is_err()) return r;
    mags.assign(frames, std::vector<float>());
    for (size_t f = 0; f < frames; ++f) mags[f].assign(flat.begin() + f * half, flat.begin() + (f + 1) * half);
    return Result::Ok();
}

// ---- the STFT families over rows of signals (kofft_hip.h, "ROWS of signals"): `signals` holds rows * len samples, rows dense ----
// stft::stft per row into rows * frames * window.size() values; frames defaults to ceil(len / hop)
inline Result stft_rows(const std::vector<float> &signals, size_t rows, const std::vector<float> &window, size_t hop_size,
                        std::vector<Complex32> &out, const HipFftImpl<float> &fft, size_t frames = static_cast<size_t>(-1))
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);  // stft.rs:83
    if (rows == 0 || signals.size() % rows != 0) return rows == 0 && signals.empty() ? Result::Ok() : Result::Err(FftError::MismatchedLengths);
    const size_t len = signals.size() / rows;
    if (frames == static_cast<size_t>(-1)) frames = (len + hop_size - 1) / hop_size;
    out.assign(rows * frames * window.size(), Complex32{});
    return fft.st(kofft_hip_stft_rows_f32(fft.raw(), signals.data(), rows, len, len, window.data(), window.size(), hop_size,
                                          reinterpret_cast<float *>(out.data()), frames));
}
// visual::spectrogram::stft_magnitudes per row: mags rows * frames * (win_len / 2), one maximum per row
inline Result stft_magnitudes_rows(const std::vector<float> &samples, size_t rows, size_t win_len, size_t hop, std::vector<float> &mags,
                                   std::vector<float> &max_mag, const HipFftImpl<float> &fft)
{
    if (hop == 0) return Result::Err(FftError::InvalidHopSize);
    if (rows == 0 || samples.size() % rows != 0) return rows == 0 && samples.empty() ? Result::Ok() : Result::Err(FftError::MismatchedLengths);
    const size_t len = samples.size() / rows, frames = (len + hop - 1) / hop;
    mags.assign(rows * frames * (win_len / 2), 0.0f);
    max_mag.assign(rows, 0.0f);
    return fft.st(kofft_hip_stft_magnitudes_rows_f32(fft.raw(), samples.data(), rows, len, len, win_len, hop, mags.data(), frames,
                                                     max_mag.data()));
}
// stft::istft per row (frames transformed in place, scratch = the window-square sums); parallel: stft::inverse_parallel per row
// (frames untouched, scratch unused)
inline Result istft_rows(std::vector<Complex32> &frames, size_t rows, const std::vector<float> &window, size_t hop_size,
                         std::vector<float> &output, std::vector<float> &scratch, const HipFftImpl<float> &fft, bool parallel = false)
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);
    if (rows == 0) return Result::Ok();
    const size_t wl = window.size();
    if (output.size() % rows != 0 || (wl && frames.size() % (rows * wl) != 0)) return Result::Err(FftError::MismatchedLengths);
    const size_t count = wl ? frames.size() / (rows * wl) : 0, out_len = output.size() / rows;
    if (parallel)
        return fft.st(kofft_hip_istft_parallel_rows_f32(fft.raw(), reinterpret_cast<const float *>(frames.data()), rows, count, window.data(),
                                                        wl, hop_size, output.data(), out_len));
    if (scratch.size() != output.size()) return Result::Err(FftError::MismatchedLengths);  // stft.rs:128
    return fft.st(kofft_hip_istft_rows_f32(fft.raw(), reinterpret_cast<float *>(frames.data()), rows, count, window.data(), wl, hop_size,
                                           output.data(), out_len, scratch.data(), out_len));
}

// the one-sided STFT per row (kofft_hip.h, "one-sided STFT"): rows * frames * (window.size() / 2 + 1) values, bit for bit the first
// window.size() / 2 + 1 bins of every frame of stft_rows; frames defaults to ceil(len / hop)
inline Result stft_onesided(const std::vector<float> &signals, size_t rows, const std::vector<float> &window, size_t hop_size,
                            std::vector<Complex32> &out, const HipFftImpl<float> &fft, size_t frames = static_cast<size_t>(-1))
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);  // stft.rs:83
    if (rows == 0 || signals.size() % rows != 0) return rows == 0 && signals.empty() ? Result::Ok() : Result::Err(FftError::MismatchedLengths);
    const size_t len = signals.size() / rows;
    if (frames == static_cast<size_t>(-1)) frames = (len + hop_size - 1) / hop_size;
    out.assign(rows * frames * (window.size() / 2 + 1), Complex32{});
    return fft.st(kofft_hip_stft_onesided_f32(fft.raw(), signals.data(), rows, len, len, window.data(), window.size(), hop_size,
                                              reinterpret_cast<float *>(out.data()), frames));
}
// stft::inverse_parallel per row of the Hermitian completion of one-sided frames (`half`: rows * frames * (window.size() / 2 + 1)
// values, only read); output: rows * out_len, accumulated into
inline Result istft_onesided(const std::vector<Complex32> &half, size_t rows, const std::vector<float> &window, size_t hop_size,
                             std::vector<float> &output, const HipFftImpl<float> &fft)
{
    if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);
    if (rows == 0) return Result::Ok();
    const size_t wl = window.size(), bins = wl / 2 + 1;
    if (output.size() % rows != 0 || half.size() % (rows * bins) != 0) return Result::Err(FftError::MismatchedLengths);
    return fft.st(kofft_hip_istft_onesided_f32(fft.raw(), reinterpret_cast<const float *>(half.data()), rows, half.size() / (rows * bins),
                                               window.data(), wl, hop_size, output.data(), output.size() / rows));
}

// ndfft::fft2d_inplace (ndfft.rs:74-101) / fft3d_inplace (ndfft.rs:114-155): same length checks, same order
template <typename T>
Result fft2d_inplace(std::vector<Complex<T>> &data, size_t rows, size_t cols, const HipFftImpl<T> &fft,
                     std::vector<Complex<T>> &scratch_col)
{
    if (rows * cols != data.size()) return Result::Err(FftError::MismatchedLengths);
    if (rows == 0 || cols == 0) return Result::Ok();
    if (scratch_col.size() != rows) return Result::Err(FftError::MismatchedLengths);
    return fft.st(detail::Abi<T>::fftnd(fft.raw(), reinterpret_cast<T *>(data.data()), 1, rows, cols, 0));
}
template <typename T>
Result fft3d_inplace(std::vector<Complex<T>> &data, size_t depth, size_t rows, size_t cols, const HipFftImpl<T> &fft,
                     std::vector<Complex<T>> &tube, std::vector<Complex<T>> &row, std::vector<Complex<T>> &col)
{
    if (depth * rows * cols != data.size()) return Result::Err(FftError::MismatchedLengths);
    if (depth == 0 || rows == 0 || cols == 0) return Result::Ok();
    if (tube.size() != depth || row.size() != rows || col.size() != cols) return Result::Err(FftError::MismatchedLengths);
    return fft.st(detail::Abi<T>::fftnd(fft.raw(), reinterpret_cast<T *>(data.data()), depth, rows, cols, 0));
}

// Multi-GPU STFT: frames sharded over the devices of one process, optional RCCL all-gather of the
// spectra -- the device analogue of stft::parallel's rayon-over-frames (stft.rs:232-263).
class HipMulti {
public:
    explicit HipMulti(int ngpu, const int *devices = nullptr)
    {
        const int rc = kofft_hip_multi_create(ngpu, devices, &h_);
        if (rc > 0) throw std::invalid_argument("kofft_hip_multi_create: invalid device count");
        if (rc != 0) throw DeviceError(rc, "kofft_hip_multi_create");
    }
    ~HipMulti() { if (h_) kofft_hip_multi_destroy(h_); }
    HipMulti(const HipMulti &) = delete;
    HipMulti &operator=(const HipMulti &) = delete;
    int ngpu() const { return kofft_hip_multi_ngpu(h_); }
    // stft::stft's checks and result; frames [r*ceil(F/G), ...) computed by device r
    Result stft(const std::vector<float> &signal, const std::vector<float> &window, size_t hop_size,
                std::vector<std::vector<Complex32>> &output, bool allgather = false)
    {
        const size_t frames = output.size(), wl = window.size();
        std::vector<Complex32> flat(frames * wl);
        const int rc = kofft_hip_multi_stft_f32(h_, signal.data(), signal.size(), window.data(), wl, hop_size,
                                                reinterpret_cast<float *>(flat.data()), frames, allgather ? 1 : 0, nullptr);
        if (rc > 0) return Result::Err(static_cast<FftError>(rc));
        if (rc != 0) throw DeviceError(rc, kofft_hip_multi_last_error(h_));
        for (size_t f = 0; f < frames; ++f) output[f].assign(flat.begin() + f * wl, flat.begin() + (f + 1) * wl);
        return Result::Ok();
    }
    // fft::batch (fft.rs:2156-2175) over a contiguous batch, in G contiguous blocks, no exchange
    Result fft_batch(std::vector<Complex32> &data, size_t n, bool inverse = false)
    {
        return st(kofft_hip_multi_fft_c32(h_, reinterpret_cast<float *>(data.data()), n, n ? data.size() / n : 0, inverse ? 1 : 0));
    }
    Result fft_batch(std::vector<Complex64> &data, size_t n, bool inverse = false)
    {
        return st(kofft_hip_multi_fft_c64(h_, reinterpret_cast<double *>(data.data()), n, n ? data.size() / n : 0, inverse ? 1 : 0));
    }
    // rfft_direct (rfft.rs:425-465) on every row of n reals, optional window product first (BASELINE config #3's shape)
    Result rfft_batch(const std::vector<float> &rows, size_t n, std::vector<Complex32> &out, const std::vector<float> *window = nullptr)
    {
        const size_t batch = n ? rows.size() / n : 0;
        if (window && window->size() != n) return Result::Err(FftError::MismatchedLengths);
        out.resize(batch * (n / 2 + 1));
        return st(kofft_hip_multi_rfft_f32(h_, rows.data(), reinterpret_cast<float *>(out.data()), window ? window->data() : nullptr, n, batch));
    }
    // device-resident twins (one device pointer per device, asynchronous): thin pass-throughs
    Result fft_dev(float *const *d_data, size_t n, size_t batch, bool inverse = false)
    {
        return st(kofft_hip_multi_fft_c32_dev(h_, d_data, n, batch, inverse ? 1 : 0));
    }
    Result fft_dev(double *const *d_data, size_t n, size_t batch, bool inverse = false)
    {
        return st(kofft_hip_multi_fft_c64_dev(h_, d_data, n, batch, inverse ? 1 : 0));
    }
    Result rfft_dev(const float *const *d_in, float *const *d_out, const float *const *d_window, size_t n, size_t batch)
    {
        return st(kofft_hip_multi_rfft_f32_dev(h_, d_in, d_out, d_window, n, batch));
    }
    Result stft_dev(const float *const *d_signal, size_t len, const float *const *d_window, size_t win_len, size_t hop, size_t frames,
                    bool allgather, float **d_out)
    {
        return st(kofft_hip_multi_stft_f32_dev(h_, d_signal, len, d_window, win_len, hop, frames, allgather ? 1 : 0, d_out));
    }
    std::pair<size_t, size_t> shard(size_t total, int rank) const
    {
        size_t f = 0, c = 0;
        kofft_hip_multi_shard(h_, total, rank, &f, &c);
        return {f, c};
    }
    std::pair<size_t, size_t> stft_slice(size_t len, size_t win_len, size_t hop, size_t frames, int rank) const
    {
        size_t f = 0, c = 0;
        kofft_hip_multi_stft_slice(h_, len, win_len, hop, frames, rank, &f, &c);
        return {f, c};
    }
    void synchronize() { (void)st(kofft_hip_multi_synchronize(h_)); }
    struct Timing { float upload_ms = 0, kernel_ms = 0, gather_ms = 0, download_ms = 0, wall_ms = 0; };
    Timing last_timing() const
    {
        Timing t;
        kofft_hip_multi_last_timing_ex(h_, &t.upload_ms, &t.kernel_ms, &t.gather_ms, &t.download_ms, &t.wall_ms);
        return t;
    }
    // the exchange form: KOFFT_MULTI_GATHER_RCCL (grouped ncclAllGather) or KOFFT_MULTI_GATHER_DIRECT (peer copies on per-peer streams)
    Result set_gather(int mode) { return st(kofft_hip_multi_set_gather(h_, mode)); }
    int last_gather() const
    {
        int last = 0;
        kofft_hip_multi_gather_mode(h_, nullptr, &last);
        return last;
    }
    kofft_hip_multi *raw() const { return h_; }

private:
    Result st(int rc) const
    {
        if (rc > 0) return Result::Err(static_cast<FftError>(rc));
        if (rc != 0) throw DeviceError(rc, kofft_hip_multi_last_error(h_));
        return Result::Ok();
    }
    kofft_hip_multi *h_ = nullptr;
};

// stft::parallel (stft.rs:232-263): only hop == 0 is rejected
inline Result parallel(const std::vector<float> &signal, const std::vector<float> &window, size_t hop_size,
                       std::vector<std::vector<Complex32>> &output, const HipFftImpl<float> &fft)
{
    return stft(signal, window, hop_size, output, fft, false);
}
// stft::frame (stft.rs:355-372)
inline Result frame(const std::vector<float> &signal, const std::vector<float> &window, size_t start,
                    std::vector<Complex32> &frame_out, const HipFftImpl<float> &fft)
{
    if (frame_out.size() < window.size()) throw std::out_of_range("frame_out shorter than the window (the reference panics)");
    return fft.st(kofft_hip_stft_frame_f32(fft.raw(), signal.data(), signal.size(), window.data(), window.size(), start,
                                           reinterpret_cast<float *>(frame_out.data())));
}

class StftStream {  // stft.rs:160-206
public:
    static Result create(const std::vector<float> &signal, const std::vector<float> &window, size_t hop_size,
                         const HipFftImpl<float> &fft, StftStream *&out)
    {
        if (hop_size == 0) return Result::Err(FftError::InvalidHopSize);
        out = new StftStream(signal, window, hop_size, fft);
        return Result::Ok();
    }
    // Ok(true) -> *more = true
    Result next_frame(std::vector<Complex32> &out, bool &more)
    {
        more = false;
        if (out.size() != window_.size()) return Result::Err(FftError::MismatchedLengths);
        if (pos_ >= signal_.size()) return Result::Ok();
        Result r = frame(signal_, window_, pos_, out, fft_);
        if (r.is_err()) return r;
        pos_ += hop_;
        more = true;
        return Result::Ok();
    }

private:
    StftStream(const std::vector<float> &s, const std::vector<float> &w, size_t hop, const HipFftImpl<float> &f)
        : signal_(s), window_(w), hop_(hop), pos_(0), fft_(f)
    {
    }
    const std::vector<float> &signal_;
    const std::vector<float> &window_;
    size_t hop_, pos_;
    const HipFftImpl<float> &fft_;
};

// stft::IstftStream (stft.rs:401-518): streaming overlap-add with normalisation.  push_frame hands the frame to the
// device (ifft + windowed add into the ring buffer = inverse_frame's arithmetic); the window-square bookkeeping and the
// "> 1e-8" division of the samples that leave the buffer are host bookkeeping, as in the reference's helper.
class IstftStream {
public:
    static Result create(size_t win_len, size_t hop, std::vector<float> window, const HipFftImpl<float> &fft, IstftStream *&out)
    {
        if (hop == 0) return Result::Err(FftError::InvalidHopSize);
        out = new IstftStream(win_len, hop, std::move(window), fft);
        return Result::Ok();
    }
    // the next `hop` samples of the reconstructed signal
    Result push_frame(const std::vector<Complex32> &frame_in, std::vector<float> &out)
    {
        if (frame_in.size() != win_len_) return Result::Err(FftError::MismatchedLengths);
        if (window_.size() < win_len_) throw std::out_of_range("window shorter than win_len (the reference panics)");
        time_buf_ = frame_in;
        Result r = fft_.st(kofft_hip_istft_frame_f32(fft_.raw(), reinterpret_cast<float *>(time_buf_.data()), window_.data(), win_len_,
                                                     0, buffer_.data() + buf_pos_, win_len_));
        if (r.is_err()) return r;
        for (size_t i = 0; i < win_len_; ++i) norm_buf_[buf_pos_ + i] += window_[i] * window_[i];
        ++frame_count_;
        normalise(out_pos_, out_pos_ + hop_, out);
        out_pos_ += hop_;
        buf_pos_ += hop_;
        if (buf_pos_ + win_len_ > buffer_.size()) {
            buffer_.resize(buf_pos_ + win_len_, 0.0f);
            norm_buf_.resize(buf_pos_ + win_len_, 0.0f);
        }
        for (size_t i = 0; i < hop_; ++i) {
            buffer_[buf_pos_ + win_len_ - hop_ + i] = 0.0f;
            norm_buf_[buf_pos_ + win_len_ - hop_ + i] = 0.0f;
        }
        return Result::Ok();
    }
    // the remaining win_len - hop samples after the last frame (empty before the first frame and on later calls)
    void flush(std::vector<float> &out)
    {
        out.clear();
        if (frame_count_ == 0) return;
        const size_t lo = out_pos_, hi = buf_pos_ + win_len_ - hop_;
        if (lo >= hi) return;
        normalise(lo, hi, out);
        out_pos_ = hi;
    }

private:
    IstftStream(size_t win_len, size_t hop, std::vector<float> window, const HipFftImpl<float> &fft)
        : win_len_(win_len), hop_(hop), window_(std::move(window)), fft_(fft), buffer_(win_len + 2 * hop, 0.0f),
          norm_buf_(win_len + 2 * hop, 0.0f), time_buf_(win_len)
    {
    }
    void normalise(size_t lo, size_t hi, std::vector<float> &out)
    {
        out.resize(hi - lo);
        for (size_t i = lo; i < hi; ++i) {
            if (norm_buf_[i] > 1e-8f) buffer_[i] /= norm_buf_[i];
            norm_buf_[i] = 0.0f;
            out[i - lo] = buffer_[i];
        }
    }
    size_t win_len_, hop_;
    std::vector<float> window_;
    const HipFftImpl<float> &fft_;
    std::vector<float> buffer_, norm_buf_;
    std::vector<Complex32> time_buf_;
    size_t buf_pos_ = 0, out_pos_ = 0, frame_count_ = 0;
};

}  // namespace kofft
