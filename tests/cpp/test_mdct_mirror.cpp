// The C++ host mirror of the fast DCT-IV, the MDCT and the IMDCT (include/kofft_hip.hpp: dct4_fast_rows / mdct_rows / imdct_rows /
// set_mdct_fused) against the vectors tests/test_cpp_mdct_mirror.py writes (inputs and the test oracle's outputs): bit for bit on the
// default route and on the composed one, a window of the IMDCT against the whole, and the mirror's own errors.  Exit status 0 and
// " 0 failed" when every check passes.  usage: test_mdct_mirror VECTORS
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

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

static bool read_floats(std::FILE *f, std::vector<float> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
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
        uint64_t s[5];
        if (std::fread(s, sizeof(uint64_t), 5, f) != 5) break;
        const size_t n = s[0], rows = s[1], nx = s[2], lead = s[3], frames = s[4], full = (frames + 1) * n;
        float scale = 0.0f;
        if (std::fread(&scale, sizeof scale, 1, f) != 1) break;
        std::vector<float> x, w, want_d, want_X, want_y;
        if (!read_floats(f, x, rows * nx) || !read_floats(f, w, 2 * n) || !read_floats(f, want_d, rows * frames * n) ||
            !read_floats(f, want_X, rows * frames * n) || !read_floats(f, want_y, rows * full))
            break;
        for (bool fused : {true, false}) {
            std::vector<float> X, d, y, part;
            CHECK(fft.set_mdct_fused(fused).is_ok());
            CHECK(fft.mdct_rows(x, w, X, rows, lead, frames).is_ok());
            CHECK(same_bits(X, want_X));
            CHECK(fft.dct4_fast_rows(want_X, d, rows * frames).is_ok());  // the DCT-IV of the coefficients, row by row
            CHECK(same_bits(d, want_d));
            CHECK(fft.imdct_rows(want_X, w, y, rows, scale).is_ok());
            CHECK(same_bits(y, want_y));
            const size_t first = n + n / 2, count = full - first - 1;
            CHECK(fft.imdct_rows(want_X, w, part, rows, scale, first, count).is_ok() && part.size() == rows * count);
            bool same = part.size() == rows * count;
            for (size_t r = 0; r < rows && same; ++r) same = std::memcmp(&part[r * count], &want_y[r * full + first], count * sizeof(float)) == 0;
            CHECK(same);
        }
        ++done;
    }
    std::fclose(f);
    CHECK(done == cases);
    {   // the defaults, the mirror's own checks, then the C entry's in its order
        std::vector<float> x(40, 1.0f), w(16, 0.5f), none, bad(7), odd(15, 1.0f), out;
        CHECK(fft.set_mdct_fused(true).is_ok());
        CHECK(fft.mdct_rows(x, w, out, 2).is_ok() && out.size() == 2 * 4 * 8);  // nx 20, N 8: ceil(20 / 8) + 1 frames
        std::vector<float> back;
        CHECK(fft.imdct_rows(out, w, back, 2).is_ok() && back.size() == 2 * 5 * 8);
        CHECK(fft.mdct_rows(x, w, out, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.mdct_rows(bad, w, out, 2).unwrap_err() == FftError::MismatchedLengths);  // rows do not divide x
        CHECK(fft.mdct_rows(x, odd, out, 2).unwrap_err() == FftError::MismatchedLengths);  // a window of odd length
        CHECK(fft.mdct_rows(none, w, out, 1).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.mdct_rows(x, none, out, 2).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.mdct_rows(x, std::vector<float>(14, 1.0f), out, 2).unwrap_err() == FftError::InvalidValue);  // N = 7
        CHECK(fft.mdct_rows(x, w, out, 2, 16).unwrap_err() == FftError::InvalidValue);                          // lead == 2N
        CHECK(fft.mdct_rows(x, w, out, 2, 8, 0).is_ok() && out.empty());
        CHECK(fft.imdct_rows(x, w, out, 3).unwrap_err() == FftError::MismatchedLengths);  // 40 is no multiple of 3 * 8
        CHECK(fft.imdct_rows(x, w, out, 1, 1.0f, 49).unwrap_err() == FftError::MismatchedLengths);  // full = 48
        CHECK(fft.imdct_rows(x, w, out, 1, 1.0f, 40, 9).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.imdct_rows(x, w, out, 1, 1.0f, 48).is_ok() && out.empty());
        CHECK(fft.dct4_fast_rows(x, out, 3).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dct4_fast_rows(x, out, 8).unwrap_err() == FftError::InvalidValue);  // rows of 5
        CHECK(fft.dct4_fast_rows(x, out, 4).is_ok() && out.size() == 40);
    }
    std::printf("%llu cases, %d checks, %d failed\n", (unsigned long long)done, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
