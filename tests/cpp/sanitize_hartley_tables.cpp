// sanitize_hartley_tables.cpp -- the host recipes of the Hartley transform and of the windows beyond Hann (kofft_amd/csrc/tables.cpp:
// libm_trigf, dht_table_f32, window_f32, with libm_trigf.hip.h compiled for the host) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU, at the edge sizes, into exactly-sized buffers (ASan guards the ends).  Built and run by
// tests/test_hartley_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../kofft_amd/csrc/tables.h"

static float from_bits(unsigned u)
{
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

int main()
{
    int bad = 0;
    {
        // every branch of the restated sinf / cosf, the special values, and the refusal beyond the medium range
        const unsigned pats[] = {0u,          0x80000000u, 1u,          0x39800000u, 0x397fffffu, 0x3f490fdau, 0x3f490fdbu, 0x4016cbe3u, 0x4016cbe4u,
                                 0x407b53d1u, 0x407b53d2u, 0x40afeddfu, 0x40afede0u, 0x40e231d5u, 0x40e231d6u, 0x46c90e00u, 0x4dc90fdau, 0x7f800000u,
                                 0xff800000u, 0x7fc00000u};
        std::vector<float> x;
        for (unsigned p : pats) {
            x.push_back(from_bits(p));
            x.push_back(from_bits(p ^ 0x80000000u));
        }
        std::vector<float> c(x.size()), s(x.size());
        if (!kofft_tables::libm_trigf(x.data(), x.size(), c.data(), s.data())) ++bad;
        for (size_t j = 0; j < x.size(); ++j) {
            const bool finite = std::isfinite(x[j]);
            if (finite && !(std::fabs(c[j]) <= 1.0f && std::fabs(s[j]) <= 1.0f)) ++bad;
            if (!finite && !(std::isnan(c[j]) && std::isnan(s[j]))) ++bad;
        }
        if (!kofft_tables::libm_trigf(x.data(), x.size(), nullptr, s.data()) || !kofft_tables::libm_trigf(x.data(), 0, nullptr, nullptr)) ++bad;
        const float big = from_bits(0x4dc90fdbu);
        float one = 7.0f;
        if (kofft_tables::libm_trigf(&big, 1, &one, &one) || one != 7.0f) ++bad;
    }
    for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(3), size_t(129), size_t(1000)}) {
        std::vector<float> h(n * n);
        kofft_tables::dht_table_f32(n, n, h.data());
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < i; ++k)
                if (std::memcmp(&h[i * n + k], &h[k * n + i], sizeof(float)) != 0) ++bad;
        if (n && (h[0] != 1.0f || h[n - 1] != 1.0f || h[(n - 1) * n] != 1.0f)) ++bad;
    }
    {
        // a padded row stride (columns n .. ldc - 1 are +0), and the full-size table on its threads
        std::vector<float> d(size_t(5) * 128, 7.0f);
        kofft_tables::dht_table_f32(5, 128, d.data());
        for (size_t i = 0; i < 5; ++i)
            for (size_t k = 5; k < 128; ++k)
                if (d[i * 128 + k] != 0.0f || std::signbit(d[i * 128 + k])) ++bad;
        std::vector<float> h(size_t(4096) * 4096);
        kofft_tables::dht_table_f32(4096, 4096, h.data());
        if (h[0] != 1.0f || !(std::fabs(h.back()) <= 1.5f)) ++bad;
    }
    const float params[] = {0.0f, 0.5f, 1.0f, 1.5f, -0.5f, 5.0f, 8.6f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                            -std::numeric_limits<float>::infinity(), 3e38f};
    for (int kind = 0; kind < kofft_tables::kWindowKinds; ++kind) {
        for (size_t len : {size_t(0), size_t(1), size_t(2), size_t(3), size_t(8), size_t(255), size_t(4096)}) {
            if (kind == 2 && len == 0) continue;  // kaiser(0, .): refused by the C ABI (the reference underflows len - 1)
            for (float p : params) {
                std::vector<float> w(len, 7.0f);
                kofft_tables::window_f32(kind, len, p, w.data());
                if (len >= 2 && kind != 2 && kind != 3 && !std::isfinite(w[len / 2])) ++bad;
                if (kind == 3 && !(p > 0.0f))  // alpha <= 0 and a NaN alpha: all ones
                    for (float v : w)
                        if (v != 1.0f) ++bad;
            }
        }
    }
    std::printf("sanitize_hartley_tables: %d problems\n", bad);
    return bad ? 1 : 0;
}
