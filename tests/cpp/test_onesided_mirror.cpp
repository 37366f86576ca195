// The C++ host mirror of the one-sided STFT (include/kofft_hip.hpp: stft_onesided / istft_onesided) against the mirror's own stft_rows
// and istft_rows: the forward result is the prefix of every full frame bit for bit, the inverse equals inverse_parallel of the
// Hermitian completion bit for bit and leaves its input alone, and the mirror's length errors.  Exit status 0 and " 0 failed" when
// every check passes.
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

static void one_shape(const HipFftImpl<float> &fft, size_t rows, size_t len, size_t n, size_t hop)
{
    const size_t bins = n / 2 + 1, frames = (len + hop - 1) / hop;
    std::vector<float> sig(rows * len), win(n);
    for (size_t i = 0; i < sig.size(); ++i) sig[i] = (float)std::sin(0.37 * (double)i) - 0.25f * (float)std::cos(0.011 * (double)i);
    for (size_t i = 0; i < n; ++i) win[i] = 0.1f + 0.9f * (float)(0.5 - 0.5 * std::cos(6.283185307179586 * (double)i / (double)n));
    std::vector<Complex32> full, half;
    CHECK(stft_rows(sig, rows, win, hop, full, fft).is_ok());
    CHECK(stft_onesided(sig, rows, win, hop, half, fft).is_ok());
    CHECK(half.size() == rows * frames * bins && full.size() == rows * frames * n);
    bool prefix = half.size() == rows * frames * bins;
    for (size_t t = 0; prefix && t < rows * frames; ++t)
        prefix = std::memcmp(&half[t * bins], &full[t * n], bins * sizeof(Complex32)) == 0;
    CHECK(prefix);

    // inverse: the completed frames through inverse_parallel
    std::vector<Complex32> done(rows * frames * n);
    for (size_t t = 0; t < rows * frames; ++t)
        for (size_t k = 0; k < n; ++k)
            done[t * n + k] = k < bins ? half[t * bins + k] : Complex32(half[t * bins + (n - k)].re, -half[t * bins + (n - k)].im);
    const size_t out_len = (frames - 1) * hop + n;
    std::vector<float> want(rows * out_len, 0.5f), got(rows * out_len, 0.5f), none;
    const std::vector<Complex32> before = half;
    CHECK(istft_rows(done, rows, win, hop, want, none, fft, true).is_ok());
    CHECK(istft_onesided(half, rows, win, hop, got, fft).is_ok());
    CHECK(std::memcmp(want.data(), got.data(), want.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(before.data(), half.data(), half.size() * sizeof(Complex32)) == 0);
}

int main()
{
    HipFftImpl<float> fft;
    one_shape(fft, 3, 1000, 256, 64);  // a fused window
    one_shape(fft, 2, 700, 15, 4);     // the composed route and the pack kernel
    one_shape(fft, 2, 9, 1, 1);        // one bin
    {   // the mirror's own errors
        std::vector<float> sig(10, 1.0f), win(4, 1.0f), out(10);
        std::vector<Complex32> half;
        CHECK(stft_onesided(sig, 2, win, 0, half, fft) == Result::Err(FftError::InvalidHopSize));
        CHECK(stft_onesided(sig, 3, win, 2, half, fft) == Result::Err(FftError::MismatchedLengths));
        CHECK(stft_onesided(sig, 2, win, 2, half, fft, 1) == Result::Err(FftError::MismatchedLengths));  // frames < ceil(len / hop)
        half.assign(7, Complex32{});
        CHECK(istft_onesided(half, 2, win, 0, out, fft) == Result::Err(FftError::InvalidHopSize));
        CHECK(istft_onesided(half, 2, win, 2, out, fft) == Result::Err(FftError::MismatchedLengths));  // 7 is no multiple of 2 * 3
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
