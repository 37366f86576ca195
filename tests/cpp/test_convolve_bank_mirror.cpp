// The C++ host mirror of the filter-bank convolution (include/kofft_hip.hpp: convolve_bank_rows / set_convolve_bank_fused) against a
// direct sum in double, the two routes against each other bit for bit, one real filter against convolve_rows, the real part and the
// magnitude against the complex values, windows against the full result, and the mirror's length errors.  Exit status 0 and
// " 0 failed" when every check passes.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kofft_hip.hpp"

using namespace kofft;
using Cf = Complex<float>;
static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

template <typename V>
static bool same_bits(const std::vector<V> &a, const std::vector<V> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}

// full convolution (correlate: with the taps reversed and conjugated) of every row with every filter, in double
static std::vector<std::complex<double>> direct(const std::vector<float> &x, const std::vector<Cf> &h, size_t rows, size_t nh, bool correlate)
{
    const size_t nx = x.size() / rows, filters = h.size() / nh, full = nx + nh - 1;
    std::vector<std::complex<double>> out(rows * filters * full);
    for (size_t r = 0; r < rows; ++r)
        for (size_t f = 0; f < filters; ++f)
            for (size_t i = 0; i < nx; ++i)
                for (size_t j = 0; j < nh; ++j) {
                    const Cf t = h[f * nh + (correlate ? nh - 1 - j : j)];
                    out[(r * filters + f) * full + i + j] += (double)x[r * nx + i] * std::complex<double>(t.re, correlate ? -t.im : t.im);
                }
    return out;
}

static double rel_l2(const std::vector<Cf> &got, const std::vector<std::complex<double>> &want)
{
    double num = 0.0, den = 0.0;
    for (size_t i = 0; i < want.size(); ++i) {
        num += std::norm(std::complex<double>(got[i].re, got[i].im) - want[i]);
        den += std::norm(want[i]);
    }
    return std::sqrt(num / den);
}

int main()
{
    HipFftImpl<float> fft;
    const size_t rows = 3, nx = 700, nh = 65, filters = 4, full = nx + nh - 1;
    std::vector<float> x(rows * nx), hr(filters * nh);
    std::vector<Cf> hc(filters * nh);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)std::sin(0.37 * (double)i) + 0.25f * (float)std::cos(2.1 * (double)i);
    for (size_t i = 0; i < hc.size(); ++i) {
        hr[i] = (float)std::cos(0.9 * (double)i) * 0.5f;
        hc[i] = Cf(hr[i], (float)std::sin(1.3 * (double)i) * 0.5f);
    }
    for (size_t block : {(size_t)0, (size_t)256, (size_t)128, (size_t)16384}) {  // 0: the default (1024: one block per row)
        // the oracle's error bound against float64 at this block (tests/test_convolve_bank_cpu.py): 1e-6 + 2e-7 * block
        const double bound = 1e-6 + 2e-7 * (double)(block ? block : 1024);
        for (bool correlate : {false, true}) {
            std::vector<Cf> c, c_c;
            std::vector<float> re, re_c, mag, mag_c;
            CHECK(fft.set_convolve_bank_fused(true).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, c, rows, block, 0, SIZE_MAX, correlate).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, re, rows, block, 0, SIZE_MAX, correlate).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, mag, rows, block, 0, SIZE_MAX, correlate, true).is_ok());
            CHECK(fft.set_convolve_bank_fused(false).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, c_c, rows, block, 0, SIZE_MAX, correlate).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, re_c, rows, block, 0, SIZE_MAX, correlate).is_ok());
            CHECK(fft.convolve_bank_rows(x, hc, nh, mag_c, rows, block, 0, SIZE_MAX, correlate, true).is_ok());
            CHECK(c.size() == rows * filters * full && same_bits(c, c_c) && same_bits(re, re_c) && same_bits(mag, mag_c));
            CHECK(rel_l2(c, direct(x, hc, rows, nh, correlate)) <= bound);
            bool parts = re.size() == c.size() && mag.size() == c.size();
            for (size_t i = 0; i < c.size() && parts; ++i) {
                const float m = std::sqrt(c[i].re * c[i].re + c[i].im * c[i].im);  // (built with -ffp-contract=off: un-fused)
                parts = std::memcmp(&re[i], &c[i].re, 4) == 0 && (std::memcmp(&mag[i], &m, 4) == 0 || (std::isnan(m) && std::isnan(mag[i])));
            }
            CHECK(parts);
            // windows: "same", "valid", one sample, from mid-block to mid-block -- the full result's values
            CHECK(fft.set_convolve_bank_fused(true).is_ok());
            const size_t windows[4][2] = {{(nh - 1) / 2, nx}, {nh - 1, nx - nh + 1}, {391, 1}, {100, 300}};
            for (const auto &w : windows) {
                std::vector<Cf> part;
                CHECK(fft.convolve_bank_rows(x, hc, nh, part, rows, block, w[0], w[1], correlate).is_ok() && part.size() == rows * filters * w[1]);
                bool same = true;
                for (size_t r = 0; r < rows * filters && same; ++r)
                    same = std::memcmp(&part[r * w[1]], &c[r * full + w[0]], w[1] * sizeof(Cf)) == 0;
                CHECK(same);
            }
            // real taps, the real part: filter f of the bank is convolve_rows / correlate_rows with that filter alone
            std::vector<float> bank;
            CHECK(fft.convolve_bank_rows(x, hr, nh, bank, rows, block, 0, SIZE_MAX, correlate).is_ok() && bank.size() == rows * filters * full);
            for (size_t f = 0; f < filters; ++f) {
                const std::vector<float> one_h(hr.begin() + f * nh, hr.begin() + (f + 1) * nh);
                std::vector<float> one;
                CHECK((correlate ? fft.correlate_rows(x, one_h, nh, one, rows, block) : fft.convolve_rows(x, one_h, nh, one, rows, block)).is_ok());
                bool same = one.size() == rows * full;
                for (size_t r = 0; r < rows && same; ++r)
                    same = std::memcmp(&bank[(r * filters + f) * full], &one[r * full], full * sizeof(float)) == 0;
                CHECK(same);
            }
        }
    }
    {   // the mirror's own checks, then the C entry's in its order
        std::vector<float> out, none, bad(7);
        std::vector<Cf> cout_;
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.convolve_bank_rows(bad, hr, nh, out, 2).unwrap_err() == FftError::MismatchedLengths);   // rows do not divide x
        CHECK(fft.convolve_bank_rows(x, bad, nh, out, rows).unwrap_err() == FftError::MismatchedLengths);  // nh does not divide the bank
        CHECK(fft.convolve_bank_rows(none, hr, nh, out, 1).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.convolve_bank_rows(x, none, 0, out, rows).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.convolve_bank_rows(x, hr, nh, cout_, rows, 0, 0, SIZE_MAX, false, true).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, rows, 96).unwrap_err() == FftError::NonPowerOfTwoNoStd);
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, rows, 64).unwrap_err() == FftError::MismatchedLengths);  // block < nh
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, rows, 0, full, 1).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, rows, 0, full + 1).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.convolve_bank_rows(x, hr, nh, out, rows, 0, full, 0).is_ok() && out.empty());
        CHECK(fft.convolve_bank_rows(x, none, nh, out, rows).is_ok() && out.empty());  // no filters: nothing to do
        bool threw = false;
        try {
            (void)fft.convolve_bank_rows(x, hr, nh, out, rows, (size_t)1 << 17);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
