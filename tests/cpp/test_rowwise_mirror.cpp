// The C++ host mirror's row-wise methods (include/kofft_hip.hpp: dct2, hilbert_analytic, real_cepstrum, dct_direct, dst_direct)
// against the library's C ABI and the C oracle.  dct_direct / dst_direct: every output against ko_direct_f32 (oracle/kofft_oracle.h),
// bit for bit; the others: byte for byte against the same call made through the C ABI on another context.  Then the error results
// the header documents.  Exit status 0 and " 0 failed" when every check passes.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/kofft_hip.hpp"

extern "C" int ko_direct_f32(int family, int type, const float *x, float *out, size_t n, size_t batch);

using namespace kofft;
static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

template <typename A, typename B>
static bool same_bytes(const std::vector<A> &a, const std::vector<B> &b)
{
    return a.size() * sizeof(A) == b.size() * sizeof(B) && std::memcmp(a.data(), b.data(), a.size() * sizeof(A)) == 0;
}

static std::vector<float> rows(size_t count, unsigned seed)
{
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> x(count);
    for (auto &v : x) v = u(g);
    return x;
}

int main()
{
    HipFftImpl<float> fft;
    kofft_hip_ctx *c = nullptr;
    if (kofft_hip_create(0, &c) != 0) {
        std::printf("FAIL kofft_hip_create\n");
        return 1;
    }
    // (n, batch): the fused range and its edges, non-powers of two for dct2, one composed length past 4096
    const size_t shapes[][2] = {{1, 3}, {2, 5}, {32, 7}, {1024, 9}, {4096, 2}, {8192, 3}, {1000, 4}, {33, 130}};
    for (auto &s : shapes) {
        const size_t n = s[0], b = s[1];
        const std::vector<float> x = rows(n * b, unsigned(n * 31 + b));
        std::vector<float> y(n * b), w(n * b);
        CHECK(fft.dct2(x, y, b).is_ok());
        CHECK(kofft_hip_dct2_f32(c, x.data(), w.data(), n, b) == 0 && same_bytes(y, w));
        if (n & (n - 1)) continue;
        std::vector<Complex<float>> h(n * b);
        std::vector<float> hw(2 * n * b);
        CHECK(fft.hilbert_analytic(x, h, b).is_ok());
        CHECK(kofft_hip_hilbert_f32(c, x.data(), hw.data(), n, b) == 0 && same_bytes(h, hw));
        CHECK(fft.real_cepstrum(x, y, b).is_ok());
        CHECK(kofft_hip_cepstrum_f32(c, x.data(), w.data(), n, b) == 0 && same_bytes(y, w));
        std::vector<float> z = x;  // input and output the same vector
        CHECK(fft.real_cepstrum(z, z, b).is_ok() && same_bytes(z, w));
    }
    for (int family = 0; family < 2; ++family) {
        for (int type = 1; type <= 4; ++type) {
            for (auto &s : {std::pair<size_t, size_t>{1, 2}, {5, 3}, {64, 129}, {129, 64}, {700, 3}}) {
                const size_t n = s.first, b = s.second;
                const std::vector<float> x = rows(n * b, unsigned(1000 * family + 100 * type + n));
                std::vector<float> y(n * b), want(n * b);
                CHECK(ko_direct_f32(family, type, x.data(), want.data(), n, b) == 0);
                CHECK((family ? fft.dst_direct(type, x, y, b) : fft.dct_direct(type, x, y, b)).is_ok() && same_bytes(y, want));
                std::vector<float> z = x;  // in place, as the reference's batch_* work
                CHECK((family ? fft.dst_direct(type, z, z, b) : fft.dct_direct(type, z, z, b)).is_ok() && same_bytes(z, want));
            }
        }
    }
    {   // the error results the header documents
        const std::vector<float> x6(6, 1.0f), x8(8, 1.0f), empty;
        std::vector<float> y6(6), y8(8), y7(7), yempty;
        std::vector<Complex<float>> h6(6), h7(7), h0;
        CHECK(fft.dct2(x8, y7).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dct2(x8, y8, 3).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dct2(x8, y8, 0).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dct2(empty, yempty).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.dct2(x6, y6).is_ok());  // any length
        CHECK(fft.hilbert_analytic(x8, h7).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.hilbert_analytic(empty, h0).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.hilbert_analytic(x6, h6).unwrap_err() == FftError::NonPowerOfTwoNoStd);
        CHECK(fft.real_cepstrum(x8, y7).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.real_cepstrum(empty, yempty).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.real_cepstrum(x6, y6).unwrap_err() == FftError::NonPowerOfTwoNoStd);
        for (int t : {0, 5, -1}) {
            CHECK(fft.dct_direct(t, x8, y8).unwrap_err() == FftError::InvalidValue);
            CHECK(fft.dst_direct(t, x8, y8).unwrap_err() == FftError::InvalidValue);
        }
        CHECK(fft.dct_direct(2, x8, y7).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dst_direct(1, x8, y8, 3).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.dct_direct(3, empty, yempty).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.dst_direct(3, empty, yempty).unwrap_err() == FftError::EmptyInput);
        CHECK(fft.dct_direct(1, empty, yempty).is_ok() && fft.dst_direct(4, empty, yempty).is_ok());
        bool threw = false;
        try {
            std::vector<float> big(4097, 1.0f), out(4097);
            (void)fft.dct_direct(2, big, out);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);  // n > 4096: the table bound
    }
    kofft_hip_destroy(c);
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
