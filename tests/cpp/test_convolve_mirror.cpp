// The C++ host mirror of the overlap-save convolution (include/kofft_hip.hpp: convolve_rows / correlate_rows / set_convolve_fused)
// against a direct sum in double, the two routes against each other bit for bit, windows against the full result, and the mirror's
// length errors.  Exit status 0 and " 0 failed" when every check passes.
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

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

// full convolution (correlate: with the taps reversed) of every row, in double; per_row: row r's taps at h + r * nh
static std::vector<double> direct(const std::vector<float> &x, const std::vector<float> &h, size_t rows, size_t nh, bool per_row, bool correlate)
{
    const size_t nx = x.size() / rows, full = nx + nh - 1;
    std::vector<double> out(rows * full, 0.0);
    for (size_t r = 0; r < rows; ++r)
        for (size_t i = 0; i < nx; ++i)
            for (size_t j = 0; j < nh; ++j) {
                const float tap = h[(per_row ? r * nh : 0) + (correlate ? nh - 1 - j : j)];
                out[r * full + i + j] += (double)x[r * nx + i] * (double)tap;
            }
    return out;
}

static double rel_l2(const std::vector<float> &got, const std::vector<double> &want)
{
    double num = 0.0, den = 0.0;
    for (size_t i = 0; i < want.size(); ++i) {
        num += ((double)got[i] - want[i]) * ((double)got[i] - want[i]);
        den += want[i] * want[i];
    }
    return std::sqrt(num / den);
}

int main()
{
    HipFftImpl<float> fft;
    const size_t rows = 3, nx = 700, nh = 65, full = nx + nh - 1;
    std::vector<float> x(rows * nx), h1(nh), hr(rows * nh);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (float)std::sin(0.37 * (double)i) + 0.25f * (float)std::cos(2.1 * (double)i);
    for (size_t i = 0; i < hr.size(); ++i) hr[i] = (float)std::cos(0.9 * (double)i) * 0.5f;
    for (size_t i = 0; i < nh; ++i) h1[i] = hr[i];
    for (size_t block : {(size_t)0, (size_t)256, (size_t)128, (size_t)16384}) {  // 0: the default (1024: one block per row)
        // the oracle's error bound against float64 at this block (tests/test_convolve_cpu.py): 1e-6 + 2e-7 * block
        const double bound = 1e-6 + 2e-7 * (double)(block ? block : 1024);
        for (bool per_row : {false, true}) {
            const std::vector<float> &h = per_row ? hr : h1;
            std::vector<float> conv, conv_c, corr, corr_c;
            CHECK(fft.set_convolve_fused(true).is_ok());
            CHECK(fft.convolve_rows(x, h, nh, conv, rows, block).is_ok());
            CHECK(fft.correlate_rows(x, h, nh, corr, rows, block).is_ok());
            CHECK(fft.set_convolve_fused(false).is_ok());
            CHECK(fft.convolve_rows(x, h, nh, conv_c, rows, block).is_ok());
            CHECK(fft.correlate_rows(x, h, nh, corr_c, rows, block).is_ok());
            CHECK(conv.size() == rows * full && same_bits(conv, conv_c) && same_bits(corr, corr_c));
            CHECK(rel_l2(conv, direct(x, h, rows, nh, per_row, false)) <= bound);
            CHECK(rel_l2(corr, direct(x, h, rows, nh, per_row, true)) <= bound);
            // windows: "same", "valid", one sample, from mid-block to mid-block -- the full result's values
            CHECK(fft.set_convolve_fused(true).is_ok());
            const size_t windows[4][2] = {{(nh - 1) / 2, nx}, {nh - 1, nx - nh + 1}, {391, 1}, {100, 300}};
            for (const auto &w : windows) {
                std::vector<float> part;
                CHECK(fft.convolve_rows(x, h, nh, part, rows, block, w[0], w[1]).is_ok() && part.size() == rows * w[1]);
                bool same = true;
                for (size_t r = 0; r < rows && same; ++r)
                    same = std::memcmp(&part[r * w[1]], &conv[r * full + w[0]], w[1] * sizeof(float)) == 0;
                CHECK(same);
            }
        }
    }
    {   // the mirror's own checks, then the C entry's in its order
        std::vector<float> out, none, bad(7);
        CHECK(fft.convolve_rows(x, h1, nh, out, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.convolve_rows(bad, h1, nh, out, 2).unwrap_err() == FftError::MismatchedLengths);   // rows do not divide x
        CHECK(fft.convolve_rows(x, bad, nh, out, rows).unwrap_err() == FftError::MismatchedLengths);  // taps of another size
        CHECK(fft.convolve_rows(none, h1, nh, out, 1).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.convolve_rows(x, none, 0, out, rows).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.convolve_rows(x, h1, nh, out, rows, 96).unwrap_err() == FftError::NonPowerOfTwoNoStd);
        CHECK(fft.convolve_rows(x, h1, nh, out, rows, 64).unwrap_err() == FftError::MismatchedLengths);  // block < nh
        CHECK(fft.convolve_rows(x, h1, nh, out, rows, 0, full, 1).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.correlate_rows(x, h1, nh, out, rows, 0, full + 1).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.convolve_rows(x, h1, nh, out, rows, 0, full, 0).is_ok() && out.empty());
        bool threw = false;
        try {
            (void)fft.convolve_rows(x, h1, nh, out, rows, (size_t)1 << 17);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
