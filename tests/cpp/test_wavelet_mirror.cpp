// The reference's wavelet tests (wavelet.rs:569-732) restated in C++ against the C++ host mirror (include/kofft_hip.hpp), plus
// the mirror's argument errors.  Exit status 0 and " 0 failed" when every check passes.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/kofft_hip.hpp"

using namespace kofft;
static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static float max_abs_diff(const std::vector<float> &a, const std::vector<float> &b)
{
    float m = 0.0f;
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::fabs(a[i] - b[i]));
    return m;
}

int main()
{
    HipFftImpl<float> fft;
    {   // wavelet.rs:572-580 test_haar_wavelet_roundtrip
        const std::vector<float> x = {1, 2, 3, 4};
        std::vector<float> a, d, y;
        CHECK(fft.dwt(KOFFT_WAVELET_HAAR, x, a, d).is_ok() && a.size() == 2 && d.size() == 2);
        CHECK(fft.idwt(KOFFT_WAVELET_HAAR, a, d, y).is_ok() && y.size() == 4 && max_abs_diff(x, y) < 1e-5f);
    }
    {   // wavelet.rs:602-647 db2 batch (max_err < max_val) and the strict haar batch round trip
        const std::vector<float> xs = {1, 2, 3, 4, 5, 6, 7, 8, 5, 6, 7, 8, 1, 2, 3, 4};
        std::vector<float> a, d, y;
        CHECK(fft.dwt(KOFFT_WAVELET_DB2, xs, a, d, 2).is_ok() && fft.idwt(KOFFT_WAVELET_DB2, a, d, y, 2).is_ok());
        CHECK(y.size() == xs.size() && max_abs_diff(xs, y) < 8.0f);
        CHECK(fft.dwt(KOFFT_WAVELET_HAAR, xs, a, d, 2).is_ok() && fft.idwt(KOFFT_WAVELET_HAAR, a, d, y, 2).is_ok());
        CHECK(max_abs_diff(xs, y) < 1e-6f);
    }
    {   // wavelet.rs:654-662 test_haar_multi_roundtrip and 720-731 the sym4 / coif1 multi-level lengths
        const std::vector<float> x = {1, 2, 3, 4, 5, 6, 7, 8};
        std::vector<float> a, y;
        std::vector<std::vector<float>> ds;
        CHECK(fft.dwt_multi(KOFFT_WAVELET_HAAR, x, 3, a, ds).is_ok() && a.size() == 1 && ds.size() == 3 && ds[0].size() == 4);
        CHECK(fft.idwt_multi(KOFFT_WAVELET_HAAR, a, ds, y).is_ok() && max_abs_diff(x, y) < 1e-5f);
        for (int w : {KOFFT_WAVELET_SYM4, KOFFT_WAVELET_COIF1}) {
            CHECK(fft.dwt_multi(w, x, 2, a, ds).is_ok() && fft.idwt_multi(w, a, ds, y).is_ok() && y.size() == x.size());
        }
    }
    {   // wavelet.rs:685-694 test_multi_level_batch_roundtrip (levels 2, two rows)
        const std::vector<float> xs = {1, 2, 3, 4, 5, 6, 7, 8};
        std::vector<float> a, y;
        std::vector<std::vector<float>> ds;
        CHECK(fft.dwt_multi(KOFFT_WAVELET_HAAR, xs, 2, a, ds, 2).is_ok() && fft.idwt_multi(KOFFT_WAVELET_HAAR, a, ds, y, 2).is_ok());
        CHECK(max_abs_diff(xs, y) < 1e-5f);
    }
    {   // errors: unknown wavelet, rows that do not divide, a detail shorter than the approximation (the reference panics)
        std::vector<float> a, d, y;
        std::vector<std::vector<float>> ds;
        CHECK(fft.dwt(7, {1, 2}, a, d).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.dwt(KOFFT_WAVELET_DB4, {1, 2, 3}, a, d, 2).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.idwt(KOFFT_WAVELET_DB4, {1, 2}, {1}, y).unwrap_err() == FftError::MismatchedLengths);
        // a longer detail: the entries past n are ignored, as in the reference
        std::vector<float> y2;
        CHECK(fft.idwt(KOFFT_WAVELET_DB4, {1, 2, 3, 4}, {5, 6, 9, 7, 8, 9}, y, 2).is_ok() && y.size() == 8);
        CHECK(fft.idwt(KOFFT_WAVELET_DB4, {1, 2, 3, 4}, {5, 6, 7, 8}, y2, 2).is_ok() && y == y2);
        // levels and lengths the C ABI refuses: UNSUPPORTED (DeviceError) before anything is allocated
        bool threw = false;
        try {
            (void)fft.dwt_multi(KOFFT_WAVELET_DB4, {1, 2, 3, 4}, size_t(1) << 40, a, ds);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            (void)fft.idwt_multi(KOFFT_WAVELET_HAAR, {1, 2}, std::vector<std::vector<float>>(65, std::vector<float>(2, 0.0f)), y);
        } catch (const DeviceError &) {
            threw = true;
        }
        CHECK(threw);
        CHECK(fft.dwt_multi(KOFFT_WAVELET_DB4, std::vector<float>(10, 1.0f), 2, a, ds).is_ok());  // lengths 5, 3: 5 is odd
        CHECK(ds.size() == 2 && ds[0].size() == 5 && ds[1].size() == 3 && a.size() == 3);
        CHECK(fft.idwt_multi(KOFFT_WAVELET_DB4, a, ds, y).unwrap_err() == FftError::MismatchedLengths);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
