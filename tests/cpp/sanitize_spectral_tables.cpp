// sanitize_spectral_tables.cpp -- the host recipes of the chirp-Z transform and the Goertzel detector (kofft_amd/csrc/tables.cpp:
// czt_wpow_f32, czt_apow_f32, czt_table_f32, goertzel_coeff_f32) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, at
// the edge sizes, into exactly-sized buffers (ASan guards the ends).  Built and run by tests/test_spectral_cpu.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/tables.h"

int main()
{
    int bad = 0;
    const float ws[][4] = {{0.0f, -1.0f, 1.0f, 0.0f}, {0.99f, 0.01f, 0.0f, 0.0f}, {1.5f, 0.2f, 0.7f, -0.7f}};
    for (const auto &p : ws) {
        for (size_t n : {size_t(0), size_t(1), size_t(4096)}) {
            std::vector<float> wpow(2 * n), apow(2 * n);
            kofft_tables::czt_wpow_f32(n, p[0], p[1], wpow.data());
            kofft_tables::czt_apow_f32(n, p[2], p[3], apow.data());
            if (n && (wpow[0] != 1.0f || wpow[1] != 0.0f || apow[0] != 1.0f || apow[1] != 0.0f)) ++bad;
        }
        for (size_t n : {size_t(0), size_t(1), size_t(4096)}) {
            for (size_t m : {size_t(0), size_t(1), size_t(4096)}) {
                if (n * m > 4096) continue;  // the large corners one at a time below
                std::vector<float> c(n * 2 * m);
                kofft_tables::czt_table_f32(n, m, p[0], p[1], p[2], p[3], 2 * m, c.data());
                if (n && m && (c[0] != 1.0f || c[1] != 0.0f)) ++bad;
            }
        }
    }
    {
        // the full-size table, tight and with a padded row stride (columns 2 m .. ldc - 1 are +0)
        std::vector<float> c(size_t(4096) * 2 * 4096);
        kofft_tables::czt_table_f32(4096, 4096, 0.0f, -1.0f, 1.0f, 0.0f, 2 * 4096, c.data());
        std::vector<float> d(size_t(5) * 128, 7.0f);
        kofft_tables::czt_table_f32(5, 3, 0.0f, -1.0f, 1.0f, 0.0f, 128, d.data());
        for (size_t i = 0; i < 5; ++i)
            for (size_t k = 6; k < 128; ++k)
                if (d[i * 128 + k] != 0.0f || std::signbit(d[i * 128 + k])) ++bad;
    }
    for (size_t nfreq : {size_t(0), size_t(1), size_t(1024)}) {
        std::vector<float> f(nfreq), coeff(nfreq);
        for (size_t j = 0; j < nfreq; ++j) f[j] = -4000.0f + 20.0f * (float)j;
        for (size_t n : {size_t(1), size_t(4096), size_t(1) << 26}) {
            kofft_tables::goertzel_coeff_f32(n, 8000.0f, f.data(), nfreq, coeff.data());
            for (size_t j = 0; j < nfreq; ++j)
                if (!(std::fabs(coeff[j]) <= 2.0f)) ++bad;
            kofft_tables::goertzel_coeff_f32(n, NAN, f.data(), nfreq, coeff.data());
        }
    }
    std::printf("sanitize_spectral_tables: %d problems\n", bad);
    return bad ? 1 : 0;
}
