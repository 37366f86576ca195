// The C++ host mirror of the polyphase filter bank (include/kofft_hip.hpp: pfb_analysis_rows / pfb_synthesis_rows / set_pfb_fused /
// pfb_taps / pfb_reconstruction) against the vectors tests/test_cpp_pfb_mirror.py writes (inputs and the test oracle's outputs): bit
// for bit on the default, the composed and the fused-wherever route, a window of the synthesis against the whole, and the mirror's own errors.
// Exit status 0 and " 0 failed" when every check passes.  usage: test_pfb_mirror VECTORS
#include <cstdint>
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

template <class V>
static bool read_values(std::FILE *f, std::vector<V> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::printf("usage: %s VECTORS\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    HipFftImpl<float> fft;
    uint64_t cases = 0;
    CHECK(std::fread(&cases, sizeof cases, 1, f) == 1);
    uint64_t done = 0;
    for (uint64_t c = 0; c < cases; ++c) {
        uint64_t s[8];
        if (std::fread(s, sizeof(uint64_t), 8, f) != 8) break;
        const size_t m = s[0], taps = s[1], hop = s[2], rows = s[3], nx = s[4], lead = s[5], frames = s[6], bins = s[7];
        const size_t nh = taps * m, full = (frames - 1) * hop + nh;
        float scale = 0.0f;
        if (std::fread(&scale, sizeof scale, 1, f) != 1) break;
        std::vector<float> x, h, want_y;
        std::vector<Complex<float>> want_Z;
        if (!read_values(f, x, rows * nx) || !read_values(f, h, nh) || !read_values(f, want_Z, rows * frames * bins) ||
            !read_values(f, want_y, rows * full))
            break;
        for (int fused : {1, 0, 2}) {  // the measured choice, composed, fused wherever it exists
            std::vector<Complex<float>> Z;
            std::vector<float> y, part;
            CHECK(fft.set_pfb_fused(fused).is_ok());
            CHECK(fft.pfb_analysis_rows(x, h, m, Z, rows, hop, lead, frames, bins).is_ok());
            CHECK(same_bits(Z, want_Z));
            CHECK(fft.pfb_synthesis_rows(want_Z, h, m, hop, bins, y, rows, scale).is_ok());
            CHECK(same_bits(y, want_y));
            const size_t first = hop + hop / 2, count = full - first - 1;
            CHECK(fft.pfb_synthesis_rows(want_Z, h, m, hop, bins, part, rows, scale, first, count).is_ok() && part.size() == rows * count);
            bool same = part.size() == rows * count;
            for (size_t r = 0; r < rows && same; ++r) same = std::memcmp(&part[r * count], &want_y[r * full + first], count * sizeof(float)) == 0;
            CHECK(same);
        }
        ++done;
    }
    std::fclose(f);
    CHECK(done == cases);
    {   // the defaults, the mirror's own checks, then the C entry's in its order
        std::vector<float> x(40, 1.0f), h(16, 0.5f), none, bad(7), y;
        std::vector<Complex<float>> Z, noz;
        CHECK(fft.set_pfb_fused(1).is_ok());
        CHECK(fft.set_pfb_fused(3).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.pfb_analysis_rows(x, h, 8, Z, 2).is_ok() && Z.size() == 2 * 3 * 5);  // nx 20, hop 8: ceil(20 / 8) frames of 8 / 2 + 1 bins
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 5, y, 2).is_ok() && y.size() == 2 * (2 * 8 + 16));
        CHECK(fft.pfb_analysis_rows(x, h, 8, Z, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.pfb_analysis_rows(bad, h, 8, Z, 2).unwrap_err() == FftError::MismatchedLengths);  // rows do not divide x
        CHECK(fft.pfb_analysis_rows(none, h, 8, Z, 1).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.pfb_analysis_rows(x, none, 8, Z, 2).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.pfb_analysis_rows(x, h, 0, Z, 2).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.pfb_analysis_rows(x, h, 7, Z, 2).unwrap_err() == FftError::InvalidValue);             // 16 taps, 7 channels
        CHECK(fft.pfb_analysis_rows(x, h, 8, Z, 2, 8, 16).unwrap_err() == FftError::InvalidValue);      // lead == nh
        CHECK(fft.pfb_analysis_rows(x, h, 8, Z, 2, 8, 0, 3, 9).unwrap_err() == FftError::InvalidValue);  // bins > channels
        CHECK(fft.pfb_analysis_rows(x, h, 8, Z, 2, 8, 0, 0).is_ok() && Z.empty());
        Z.assign(30, Complex<float>{});
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 4, y, 2).unwrap_err() == FftError::InvalidValue);       // bins neither 8 nor 5
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 5, y, 4).unwrap_err() == FftError::MismatchedLengths);  // 30 is no multiple of 4 * 5
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 0, 5, y, 2).unwrap_err() == FftError::InvalidHopSize);
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 5, y, 2, 1.0f, 33).unwrap_err() == FftError::MismatchedLengths);  // full = 32
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 5, y, 2, 1.0f, 30, 3).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.pfb_synthesis_rows(Z, h, 8, 8, 5, y, 2, 1.0f, 32).is_ok() && y.empty());
        CHECK(fft.pfb_synthesis_rows(Z, none, 8, 8, 5, y, 2).unwrap_err() == FftError::EmptyInput);
        int err = 0;
        const std::vector<float> p = HipFftImpl<float>::pfb_taps(8, 4, 5.0, &err);
        CHECK(err == 0 && p.size() == 32);
        double sum = 0.0;
        for (float v : p) sum += v;
        CHECK(sum > 0.999999 && sum < 1.000001);
        CHECK(HipFftImpl<float>::pfb_taps(8, 0, 5.0, &err).empty() && err == KOFFT_ERR_EMPTY_INPUT);
        CHECK(HipFftImpl<float>::pfb_taps(8, 4, -1.0, &err).empty() && err == KOFFT_ERR_INVALID_VALUE);
        double cc = 0.0, worst = 1.0;
        const std::vector<float> ones(8, 1.0f);  // the rectangular window at hop = channels reconstructs exactly, c = 1
        CHECK(HipFftImpl<float>::pfb_reconstruction(ones, ones, 8, 8, cc, worst) == 0 && cc == 1.0 && worst == 0.0);
        CHECK(HipFftImpl<float>::pfb_reconstruction(ones, h, 8, 8, cc, worst) == KOFFT_ERR_MISMATCHED_LENGTHS);
    }
    std::printf("%llu cases, %d checks, %d failed\n", (unsigned long long)done, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
