// The C++ host mirror of the Welch power spectra and cross spectra (include/kofft_hip.hpp: welch / csd / set_welch_fused / welch_scale)
// against a direct DFT in double summed over the frames, the three routes against each other bit for bit, csd(x, x) against welch(x),
// and the mirror's length errors.  Exit status 0 and " 0 failed" when every check passes.
#include <cmath>
#include <complex>
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

template <class V>
static bool same_bits(const std::vector<V> &a, const std::vector<V> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}

// sum over frames of conj(X[k]) Y[k] (x == y: |X[k]|^2) in double, scaled, the interior bins doubled; zeros past the end of a row
static std::vector<std::complex<double>> direct(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &w, size_t rows,
                                                size_t hop, size_t frames, double scale, bool twice)
{
    const size_t len = x.size() / rows, n = w.size(), K = n / 2 + 1;
    const double pi = std::acos(-1.0);
    std::vector<std::complex<double>> out(rows * K);
    for (size_t r = 0; r < rows; ++r)
        for (size_t k = 0; k < K; ++k) {
            std::complex<double> acc = 0.0;
            for (size_t f = 0; f < frames; ++f) {
                std::complex<double> X = 0.0, Y = 0.0;
                for (size_t i = 0; i < n && f * hop + i < len; ++i) {
                    const std::complex<double> e = std::polar(1.0, -2.0 * pi * (double)((k * i) % n) / (double)n);
                    X += (double)x[r * len + f * hop + i] * (double)w[i] * e;
                    Y += (double)y[r * len + f * hop + i] * (double)w[i] * e;
                }
                acc += std::conj(X) * Y;
            }
            const bool interior = k >= 1 && k < ((n & 1) ? K : K - 1);
            out[r * K + k] = acc * scale * ((twice && interior) ? 2.0 : 1.0);
        }
    return out;
}

int main()
{
    HipFftImpl<float> fft;
    const size_t rows = 3;
    // (win_len, hop, frames): a fused length with three groups, a Bluestein length, an odd length
    const size_t shapes[3][3] = {{256, 64, 70}, {100, 40, 33}, {5, 3, 40}};
    for (const auto &s : shapes) {
        const size_t win_len = s[0], hop = s[1], frames = s[2], len = (frames - 1) * hop + win_len - 3, K = win_len / 2 + 1;
        std::vector<float> x(rows * len), y(rows * len), w(win_len), none;
        for (size_t i = 0; i < x.size(); ++i) {
            x[i] = (float)std::sin(0.37 * (double)i) + 0.25f * (float)std::cos(2.1 * (double)i);
            y[i] = (float)std::cos(0.11 * (double)i) - 0.5f * (float)std::sin(1.3 * (double)i);
        }
        for (size_t i = 0; i < win_len; ++i) w[i] = 0.54f - 0.46f * (float)std::cos(2.0 * std::acos(-1.0) * (double)i / (double)win_len);
        int err = -1;
        const float scale = HipFftImpl<float>::welch_scale(w, win_len, 8000.0, frames, false, &err);
        CHECK(err == 0 && scale > 0.0f);
        for (bool twice : {false, true}) {
            std::vector<float> p[3];
            std::vector<Complex32> c[3], cxx;
            for (int mode = 0; mode < 3; ++mode) {
                CHECK(fft.set_welch_fused(mode).is_ok());
                CHECK(fft.welch(x, w, win_len, hop, frames, p[mode], rows, scale, twice).is_ok() && p[mode].size() == rows * K);
                CHECK(fft.csd(x, y, w, win_len, hop, frames, c[mode], rows, scale, twice).is_ok() && c[mode].size() == rows * K);
            }
            CHECK(same_bits(p[0], p[1]) && same_bits(p[0], p[2]) && same_bits(c[0], c[1]) && same_bits(c[0], c[2]));
            CHECK(fft.csd(x, x, w, win_len, hop, frames, cxx, rows, scale, twice).is_ok());
            bool real_same = true, imag_zero = true;
            for (size_t i = 0; i < cxx.size(); ++i) {
                real_same = real_same && std::memcmp(&cxx[i].re, &p[0][i], sizeof(float)) == 0;
                imag_zero = imag_zero && cxx[i].im == 0.0f;
            }
            CHECK(real_same && imag_zero);
            // against float64: the oracle's measured error at 1024 points, 4e-5 of the peak (tests/test_welch_cpu.py), four times that.
            // The rounding error of a cross term scales with |X| |Y|, not with the (here largely cancelling) sum: the cross spectrum is
            // measured against the geometric mean of the two power spectra's peaks.
            const auto wp = direct(x, x, w, rows, hop, frames, (double)scale, twice), wq = direct(y, y, w, rows, hop, frames, (double)scale, twice),
                       wc = direct(x, y, w, rows, hop, frames, (double)scale, twice);
            double peak_p = 0.0, peak_q = 0.0, err_p = 0.0, err_c = 0.0;
            for (size_t i = 0; i < wp.size(); ++i) {
                peak_p = std::fmax(peak_p, std::abs(wp[i]));
                peak_q = std::fmax(peak_q, std::abs(wq[i]));
                err_p = std::fmax(err_p, std::fabs((double)p[0][i] - wp[i].real()));
                err_c = std::fmax(err_c, std::abs(std::complex<double>(c[0][i].re, c[0][i].im) - wc[i]));
            }
            CHECK(err_p <= 1.6e-4 * peak_p && err_c <= 1.6e-4 * std::sqrt(peak_p * peak_q));
        }
        // a null window is window::hann(win_len): the same call with the scale of that window
        std::vector<float> ph;
        CHECK(fft.welch(x, none, win_len, hop, frames, ph, rows, HipFftImpl<float>::welch_scale(none, win_len, 1.0, frames)).is_ok());
        CHECK(ph.size() == rows * K && ph[0] >= 0.0f);
    }
    {   // the mirror's own checks, then the C entry's in its order
        std::vector<float> x(300, 1.0f), w(64, 1.0f), bad(63, 1.0f), none, out;
        std::vector<Complex32> cout_;
        CHECK(fft.welch(x, w, 64, 32, 4, out, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.welch(x, w, 64, 32, 4, out, 7).unwrap_err() == FftError::MismatchedLengths);   // rows do not divide x
        CHECK(fft.welch(x, bad, 64, 32, 4, out, 3).unwrap_err() == FftError::MismatchedLengths);  // a window of another size
        CHECK(fft.csd(x, bad, w, 64, 32, 4, cout_, 3).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.welch(x, w, 64, 0, 4, out, 3).unwrap_err() == FftError::InvalidHopSize);
        CHECK(fft.welch(x, none, 0, 32, 4, out, 3).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.welch(x, w, 64, 32, 0, out, 3).is_ok() && out.size() == 3 * 33);
        CHECK(fft.set_welch_fused(3).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.set_welch_fused(1).is_ok());
        int err = 0;
        CHECK(HipFftImpl<float>::welch_scale(w, 64, 0.0, 4, false, &err) == 0.0f && err == KOFFT_ERR_INVALID_VALUE);
        CHECK(HipFftImpl<float>::welch_scale(w, 64, 1.0, 4, true, &err) == 1.0f / (64.0f * 64.0f * 4.0f) && err == 0);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
