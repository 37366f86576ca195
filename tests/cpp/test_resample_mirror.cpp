// The C++ host mirror of the polyphase resampler (include/kofft_hip.hpp: resample_rows / set_resample_tiled / resample_taps) against
// the vectors tests/test_cpp_resample_mirror.py writes (inputs and the test oracle's outputs): bit for bit on the default route and on
// the plain one, the default count against the oracle's length, and the mirror's own errors.  Exit status 0 and " 0 failed" when every
// check passes.  usage: test_resample_mirror VECTORS
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
        uint64_t s[7];
        if (std::fread(s, sizeof(uint64_t), 7, f) != 7) break;
        const size_t up = s[0], down = s[1], rows = s[2], nx = s[3], nh = s[4], t0 = s[5], out_len = s[6];
        std::vector<float> x, h, want, got, got_plain, rest;
        if (!read_floats(f, x, rows * nx) || !read_floats(f, h, nh) || !read_floats(f, want, rows * out_len)) break;
        CHECK(fft.set_resample_tiled(true).is_ok());
        CHECK(fft.resample_rows(x, h, up, down, got, rows, t0, out_len).is_ok());
        CHECK(fft.set_resample_tiled(false).is_ok());
        CHECK(fft.resample_rows(x, h, up, down, got_plain, rows, t0, out_len).is_ok());
        CHECK(same_bits(got, want));
        CHECK(same_bits(got_plain, want));
        // the default count: every output from t0 to the end of the full result
        CHECK(fft.set_resample_tiled(true).is_ok());
        CHECK(fft.resample_rows(x, h, up, down, rest, rows, t0).is_ok());
        const size_t full_up = (nx - 1) * up + nh, count = (full_up - t0 + down - 1) / down;
        CHECK(rest.size() == rows * count && count >= out_len);
        bool same = rest.size() == rows * count;
        for (size_t r = 0; r < rows && same; ++r) same = std::memcmp(&rest[r * count], &want[r * out_len], out_len * sizeof(float)) == 0;
        CHECK(same);
        ++done;
    }
    std::fclose(f);
    CHECK(done == cases);
    {   // the mirror's own checks, then the C entry's in its order
        std::vector<float> x(20, 1.0f), h(5, 1.0f), none, bad(7), out;
        CHECK(fft.resample_rows(x, h, 1, 1, out, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.resample_rows(bad, h, 1, 1, out, 2).unwrap_err() == FftError::MismatchedLengths);  // rows do not divide x
        CHECK(fft.resample_rows(none, h, 1, 1, out, 1).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.resample_rows(x, none, 1, 1, out, 2).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.resample_rows(x, h, 0, 1, out, 2).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.resample_rows(x, h, 1, 0, out, 2, 0, 3).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.resample_rows(x, h, 1, 1, out, 2, 14, 1).unwrap_err() == FftError::MismatchedLengths);  // full_up = 14
        CHECK(fft.resample_rows(x, h, 1, 1, out, 2, 14).is_ok() && out.empty());                          // nothing left from there
        CHECK(fft.resample_rows(x, h, 1, 1, out, 2, 3, 0).is_ok() && out.empty());
        CHECK(fft.resample_rows(x, h, 2, 1, out, 2).is_ok() && out.size() == 2 * 23);
        int err = 0;
        CHECK(HipFftImpl<float>::resample_taps(3, 2).size() == 61);
        CHECK(HipFftImpl<float>::resample_taps(0, 2, 10, 5.0, &err).empty() && err == KOFFT_ERR_INVALID_VALUE);
        const std::vector<float> taps = HipFftImpl<float>::resample_taps(1, 3, 10, 5.0, &err);
        double sum = 0.0;
        for (float t : taps) sum += (double)t;
        CHECK(err == 0 && taps.size() == 61 && sum > 0.99999 && sum < 1.00001);
    }
    std::printf("%llu cases, %d checks, %d failed\n", (unsigned long long)done, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
