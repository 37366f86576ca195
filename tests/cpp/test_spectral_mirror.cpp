// The reference's chirp-Z and Goertzel tests (czt.rs:56-82, goertzel.rs:61-94) restated in C++ against the C++ host mirror
// (include/kofft_hip.hpp: czt, goertzel, set_czt_route), the batched forms against the single-row ones, and the mirror's argument
// errors.  Exit status 0 and " 0 failed" when every check passes.
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

typedef Complex32 cf;

int main()
{
    HipFftImpl<float> fft;
    const float pi = 3.14159265358979323846f;
    {   // czt.rs:60-71 test_czt_basic
        const std::vector<float> x = {1, 0, 0, 0};
        std::vector<cf> y;
        CHECK(fft.czt(x, 4, cf(std::cos(-2.0f * pi / 4.0f), std::sin(-2.0f * pi / 4.0f)), cf(1, 0), y).is_ok() && y.size() == 4);
        CHECK(std::fabs(y[0].re - 1.0f) < 1e-5f);
    }
    {   // czt.rs:73-81 test_czt_non_unit_params, under every route: the same bytes
        const std::vector<float> x = {0, 1};
        std::vector<cf> y, first;
        for (int mode : {0, 1, 2}) {
            CHECK(fft.set_czt_route(mode).is_ok());
            CHECK(fft.czt(x, 2, cf(0, 1), cf(0.5f, 0), y).is_ok() && y.size() == 2);
            CHECK(std::fabs(y[0].re - 2.0f) < 1e-5f && std::fabs(y[0].im) < 1e-5f);
            CHECK(std::fabs(y[1].re) < 1e-5f && std::fabs(y[1].im - 2.0f) < 1e-5f);
            if (mode == 0) first = y;
            CHECK(std::memcmp(first.data(), y.data(), y.size() * sizeof(cf)) == 0);
        }
        CHECK(fft.set_czt_route(3).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.set_czt_route(0).is_ok());
    }
    {   // batched rows equal the rows one by one; empty rows and m == 0
        std::vector<float> xs(3 * 70);
        for (size_t i = 0; i < xs.size(); ++i) xs[i] = std::sin(0.37f * (float)i);
        const cf w(std::cos(-0.05f), std::sin(-0.05f)), a(std::cos(0.3f), std::sin(0.3f));
        std::vector<cf> all, one;
        CHECK(fft.czt(xs, 40, w, a, all, 3).is_ok() && all.size() == 120);
        for (size_t b = 0; b < 3; ++b) {
            CHECK(fft.czt(std::vector<float>(xs.begin() + 70 * b, xs.begin() + 70 * (b + 1)), 40, w, a, one).is_ok());
            CHECK(std::memcmp(one.data(), all.data() + 40 * b, 40 * sizeof(cf)) == 0);
        }
        CHECK(fft.czt(xs, 0, w, a, all, 3).is_ok() && all.empty());
        CHECK(fft.czt(std::vector<float>(), 5, w, a, all).is_ok() && all.size() == 5 && all[4] == cf(0, 0));
        CHECK(fft.czt(xs, 4, w, a, all, 4).unwrap_err() == FftError::MismatchedLengths);
        bool threw = false;
        try {
            fft.czt(xs, 4097, w, a, all);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);
    }
    {   // goertzel.rs:65-76 test_goertzel_detects_tone, 78-93 the two errors in their order
        std::vector<float> sig(100);
        for (int i = 0; i < 100; ++i) sig[i] = std::sin(2.0f * pi * 1000.0f * (float)i / 8000.0f);
        float mag = -1.0f;
        CHECK(fft.goertzel(sig, 8000.0f, 1000.0f, mag).is_ok() && mag > 0.0f);
        CHECK(fft.goertzel(std::vector<float>(), 1.0f, 1.0f, mag).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.goertzel(std::vector<float>(), 0.0f, 1.0f, mag).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.goertzel(std::vector<float>{1.0f, 2.0f}, 0.0f, 1.0f, mag).unwrap_err() == FftError::InvalidValue);
        // batched: rows x frequencies equal the single calls
        std::vector<float> rows(4 * 100), out;
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = std::cos(0.11f * (float)i) + 0.25f * std::sin(1.7f * (float)i);
        const std::vector<float> freqs = {1000.0f, 0.0f, 4000.0f, 9000.0f, -500.0f};
        CHECK(fft.goertzel(rows, 8000.0f, freqs, out, 4).is_ok() && out.size() == 20);
        for (size_t b = 0; b < 4; ++b)
            for (size_t j = 0; j < freqs.size(); ++j) {
                float one = 0.0f;
                CHECK(fft.goertzel(std::vector<float>(rows.begin() + 100 * b, rows.begin() + 100 * (b + 1)), 8000.0f, freqs[j], one).is_ok());
                CHECK(std::memcmp(&one, &out[b * freqs.size() + j], sizeof(float)) == 0 || (std::isnan(one) && std::isnan(out[b * freqs.size() + j])));
            }
        CHECK(fft.goertzel(rows, 8000.0f, std::vector<float>(), out, 4).is_ok() && out.empty());
    }
    std::printf("test_spectral_mirror: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
