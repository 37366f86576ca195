// The reference's split-complex tests (tests/split.rs, tests/split64.rs) restated in C++ against the C++ host mirror
// (include/kofft_hip.hpp: fft_split / ifft_split, SplitComplex, ComplexVec, FftPlan), the planar entries against the interleaved ones
// bit for bit, both routes, and the mirror's length errors.  Exit status 0 and " 0 failed" when every check passes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kofft_hip.hpp"

using namespace kofft;
static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

template <typename T>
static bool same_bits(const std::vector<Complex<T>> &aos, const std::vector<T> &re, const std::vector<T> &im)
{
    for (size_t i = 0; i < aos.size(); ++i)
        if (std::memcmp(&aos[i].re, &re[i], sizeof(T)) != 0 || std::memcmp(&aos[i].im, &im[i], sizeof(T)) != 0) return false;
    return true;
}

// fft_split == fft and ifft_split == ifft on the same values, bit for bit, with the fused route on and off
template <typename T>
static void planar_equals_interleaved(const HipFftImpl<T> &fft, size_t n)
{
    std::vector<Complex<T>> aos(n);
    std::vector<T> re(n), im(n);
    for (size_t i = 0; i < n; ++i) {
        re[i] = (T)std::sin(0.37 * (double)i);
        im[i] = (T)std::cos(1.3 * (double)i) - (T)0.25;
        aos[i] = Complex<T>(re[i], im[i]);
    }
    for (bool fused : {true, false}) {
        CHECK(fft.set_split_fused(fused).is_ok());
        std::vector<Complex<T>> a = aos;
        std::vector<T> r = re, i = im;
        CHECK(fft.fft(a).is_ok() && fft.fft_split(r, i).is_ok() && same_bits(a, r, i));
        CHECK(fft.ifft(a).is_ok() && fft.ifft_split(r, i).is_ok() && same_bits(a, r, i));
    }
    CHECK(fft.set_split_fused(true).is_ok());
}

int main()
{
    HipFftImpl<float> fft;
    HipFftImpl<double> fft64;
    for (size_t n : {16, 12}) {  // split.rs:11-44 fft_split_matches_aos, fft_split_non_pow2
        std::vector<Complex32> data(n);
        for (size_t i = 0; i < n; ++i) data[i] = Complex32((float)i, 0.0f);
        std::vector<float> re(n), im(n);
        SplitComplex32 split = SplitComplex32::copy_from_complex(data, re, im);
        std::vector<Complex32> aos = data;
        CHECK(fft.fft(aos).is_ok());
        CHECK(fft_split_complex(fft, split).is_ok());
        for (size_t i = 0; i < n; ++i) CHECK(std::fabs(aos[i].re - re[i]) < 1e-6f && std::fabs(aos[i].im - im[i]) < 1e-6f);
        CHECK(same_bits(aos, re, im));
    }
    {   // split.rs:46-63 ifft_split_roundtrip
        const size_t n = 64;
        std::vector<Complex32> data(n);
        for (size_t i = 0; i < n; ++i) data[i] = Complex32((float)i, -(float)i);
        std::vector<float> re(n), im(n);
        CHECK(fft_split_complex(fft, SplitComplex32::copy_from_complex(data, re, im)).is_ok());
        CHECK(ifft_split_complex(fft, SplitComplex32(re, im)).is_ok());
        for (size_t i = 0; i < n; ++i) CHECK(std::fabs(data[i].re - re[i]) < 1e-4f && std::fabs(data[i].im - im[i]) < 1e-4f);
    }
    {   // split.rs:65-74 fft_split_errors
        std::vector<float> re(4), im(3);
        CHECK(fft_split_complex(fft, SplitComplex32(re, im)).unwrap_err() == FftError::MismatchedLengths);
        CHECK(ifft_split(fft, re, im).unwrap_err() == FftError::MismatchedLengths);
        std::vector<float> e0, e1;
        CHECK(fft_split(fft, e0, e1).unwrap_err() == FftError::EmptyInput);
        bool threw = false;
        try {
            SplitComplex32::new_(re, im);
        } catch (const std::logic_error &) {
            threw = true;
        }
        CHECK(threw);
    }
    {   // split.rs:76-93 complex_vec_roundtrip, and the FftPlan forms (fft.rs:2081-2112)
        const size_t n = 32;
        std::vector<Complex32> data(n);
        for (size_t i = 0; i < n; ++i) data[i] = Complex32((float)i, -(float)i);
        ComplexVec vec = ComplexVec::from_complex_vec(data);
        CHECK(vec.len() == n && vec.to_complex_vec() == data);
        CHECK(fft_complex_vec(fft, vec).is_ok());
        std::vector<Complex32> aos = data;
        CHECK(fft.fft(aos).is_ok() && same_bits(aos, vec.re, vec.im));
        CHECK(ifft_complex_vec(fft, vec).is_ok());
        for (size_t i = 0; i < n; ++i) CHECK(std::fabs(data[i].re - vec.re[i]) < 1e-4f && std::fabs(data[i].im - vec.im[i]) < 1e-4f);
        FftPlan<float> plan(n, FftStrategy::Auto, fft), wrong(16, FftStrategy::Auto, fft);
        ComplexVec again = ComplexVec::from_complex_vec(data);
        CHECK(plan.fft_complex_vec(again).is_ok() && same_bits(aos, again.re, again.im));
        CHECK(plan.ifft_complex_vec(again).is_ok() && again == vec);
        CHECK(wrong.fft_complex_vec(again).unwrap_err() == FftError::MismatchedLengths);
        CHECK(wrong.ifft_complex_vec(again).unwrap_err() == FftError::MismatchedLengths);
        CHECK(wrong.fft_split(again.re, again.im).unwrap_err() == FftError::MismatchedLengths);
        CHECK(wrong.ifft_split(again.re, again.im).unwrap_err() == FftError::MismatchedLengths);
        again = ComplexVec::from_complex_vec(data);
        CHECK(plan.fft_split(again.re, again.im).is_ok() && same_bits(aos, again.re, again.im));
    }
    for (size_t n : {32, 12}) {  // split64.rs:3-34
        std::vector<Complex64> aos(n);
        std::vector<double> re(n), im(n, 0.0);
        for (size_t i = 0; i < n; ++i) { aos[i] = Complex64((double)i, 0.0); re[i] = (double)i; }
        CHECK(fft64.fft(aos).is_ok() && fft_split(fft64, re, im).is_ok());
        for (size_t i = 0; i < n; ++i) CHECK(std::fabs(aos[i].re - re[i]) < 1e-10 && std::fabs(aos[i].im - im[i]) < 1e-10);
        CHECK(same_bits(aos, re, im));
    }
    {   // split64.rs:36-50 ifft_split_roundtrip_f64
        const size_t n = 64;
        std::vector<double> re(n), im(n);
        for (size_t i = 0; i < n; ++i) { re[i] = (double)i; im[i] = -(double)i; }
        CHECK(fft_split(fft64, re, im).is_ok() && ifft_split(fft64, re, im).is_ok());
        for (size_t i = 0; i < n; ++i) CHECK(std::fabs((double)i - re[i]) < 1e-8 && std::fabs(-(double)i - im[i]) < 1e-8);
    }
    for (size_t n : {1, 2, 16, 32, 100, 1024, 16384, 32768}) {
        planar_equals_interleaved(fft, n);
        planar_equals_interleaved(fft64, n);
    }
    {   // batched planes equal the rows one by one
        const size_t n = 256, batch = 5;
        std::vector<float> re(n * batch), im(n * batch);
        for (size_t i = 0; i < re.size(); ++i) { re[i] = std::sin(0.11f * (float)i); im[i] = std::cos(0.7f * (float)i); }
        std::vector<float> br = re, bi = im;
        CHECK(fft.fft_split_batch(br, bi, n).is_ok());
        for (size_t b = 0; b < batch; ++b) {
            std::vector<float> r(re.begin() + n * b, re.begin() + n * (b + 1)), i(im.begin() + n * b, im.begin() + n * (b + 1));
            CHECK(fft.fft_split(r, i).is_ok());
            CHECK(std::memcmp(r.data(), br.data() + n * b, n * sizeof(float)) == 0 && std::memcmp(i.data(), bi.data() + n * b, n * sizeof(float)) == 0);
        }
        CHECK(fft.fft_split_batch(br, bi, 7).unwrap_err() == FftError::MismatchedLengths);
    }
    std::printf("test_split_mirror: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
