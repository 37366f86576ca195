// The C++ host mirror of the IIR filter as a scan along time (include/kofft_hip.hpp: sosfilt_scan_rows / sosfilt_scan_chunk) against the
// vectors tests/test_cpp_sosfilt_scan_mirror.py writes (inputs and the scan oracle's outputs and final states): bit for bit, out of
// place and in place, and the mirror's own errors.  Exit status 0 and " 0 failed" when every check passes.
// usage: test_sosfilt_scan_mirror VECTORS
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
        uint64_t s[6];
        if (std::fread(s, sizeof(uint64_t), 6, f) != 6) break;
        const size_t rows = s[0], nx = s[1], sections = s[2], chunk = s[5];
        const bool reverse = s[3] != 0, with_zi = s[4] != 0;
        std::vector<float> x, sos, zi, want, want_zf;
        if (!read_floats(f, x, rows * nx) || !read_floats(f, sos, sections * 6) || !read_floats(f, zi, rows * sections * 2) ||
            !read_floats(f, want, rows * nx) || !read_floats(f, want_zf, rows * sections * 2))
            break;
        for (int twice = 0; twice < 2; ++twice) {
            std::vector<float> got, zf, none;
            CHECK(fft.sosfilt_scan_rows(x, sos, got, chunk, rows, with_zi ? &zi : nullptr, &zf, reverse).is_ok());
            CHECK(same_bits(got, want));
            CHECK(same_bits(zf, want_zf));
            CHECK(fft.sosfilt_scan_rows(x, sos, none, chunk, rows, with_zi ? &zi : nullptr, nullptr, reverse).is_ok());  // no final state
            CHECK(same_bits(none, want));
            std::vector<float> buf = x, state = zi;  // in place: out == x, zf == zi
            if (with_zi) {
                CHECK(fft.sosfilt_scan_rows(buf, sos, buf, chunk, rows, &state, &state, reverse).is_ok());
                CHECK(same_bits(buf, want));
                CHECK(same_bits(state, want_zf));
            }
        }
        ++done;
    }
    std::fclose(f);
    CHECK(done == cases);
    {   // the mirror's own checks, then the C entry's in its order
        std::vector<float> x(20, 1.0f), sos = {1, 0, 0, 1, 0, 0}, none, bad(7), out, short_zi(3), zf, seq;
        CHECK(fft.sosfilt_scan_rows(x, sos, out, 32, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.sosfilt_scan_rows(bad, sos, out, 32, 2).unwrap_err() == FftError::MismatchedLengths);  // rows do not divide x
        CHECK(fft.sosfilt_scan_rows(x, bad, out, 32, 2).unwrap_err() == FftError::MismatchedLengths);    // sos is no multiple of 6 values
        CHECK(fft.sosfilt_scan_rows(x, sos, out, 32, 2, &short_zi).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.sosfilt_scan_rows(x, none, out, 32, 2).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.sosfilt_scan_rows(x, sos, out, 0, 2).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.sosfilt_scan_rows(x, sos, out, 33, 2).unwrap_err() == FftError::InvalidValue);
        std::vector<float> a0 = {1, 0, 0, 2, 0, 0};
        CHECK(fft.sosfilt_scan_rows(x, a0, out, 32, 2).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.sosfilt_scan_rows(none, sos, out, 32, 1).is_ok() && out.empty());
        CHECK(fft.sosfilt_scan_rows(x, sos, out, 32, 2, nullptr, &zf).is_ok() && same_bits(out, x) && zf.size() == 4);  // the identity section
        const size_t k = HipFftImpl<float>::sosfilt_scan_chunk(2, 10, 1);
        CHECK(k >= 1024 && k % KOFFT_HIP_SOSFILT_TILE == 0);
        std::vector<float> lp = {0.25f, 0.5f, 0.25f, 1, -0.5f, 0.25f};  // one chunk holds the row: sosfilt_rows' bytes
        CHECK(fft.sosfilt_scan_rows(x, lp, out, k, 2).is_ok() && fft.sosfilt_rows(x, lp, seq, 2).is_ok() && same_bits(out, seq));
    }
    std::printf("%llu cases, %d checks, %d failed\n", (unsigned long long)done, g_checks, g_fail);
    return g_fail ? 1 : 0;
}
