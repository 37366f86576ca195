// sanitize_frontend_walk.cpp -- the per-filter walk of the fused audio front end (kofft_amd/csrc/frontend_walk.h: a lane owns one
// (frame, filter) pair) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, over plans built by kofft_tables::mel_plan_build
// into exactly-sized buffers (ASan guards the ends).  On sanitize_mel_plan.cpp's hand-made edge sets and 300 random ones every filter's
// walk must give the bits of the reference's two loops (cepstrum.rs:51-67).  Built and run by tests/test_frontend_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../kofft_amd/csrc/frontend_walk.h"
#include "../../kofft_amd/csrc/tables.h"

static int bad = 0;

static std::vector<float> two_loops(const std::vector<uint64_t> &bins, const std::vector<float> &x)
{
    const size_t num_mel = bins.size() - 2, n = x.size();
    std::vector<float> e(num_mel, 0.0f);
    for (size_t m = 1; m <= num_mel; ++m) {
        const uint64_t a = bins[m - 1], b = bins[m], c = bins[m + 1];
        if (b == a || c == b) continue;
        for (uint64_t k = a; k < b && k < n; ++k) e[m - 1] = e[m - 1] + ((float)(k - a) / (float)(b - a)) * x[k];
        for (uint64_t k = b; k < c && k < n; ++k) e[m - 1] = e[m - 1] + ((float)(c - k) / (float)(c - b)) * x[k];
    }
    return e;
}

static std::vector<float> walks(const std::vector<uint64_t> &bins, const std::vector<float> &x)
{
    const size_t num_mel = bins.size() - 2, n = x.size();
    std::vector<int> ints(kofft_tables::mel_plan_ints(num_mel));
    std::vector<float> w(2 * n);
    kofft_tables::mel_plan_build(bins.data(), n, num_mel, ints.data(), w.data());
    std::vector<float> e(num_mel, 0.0f);
    for (size_t m = num_mel; m-- > 0;)  // any order: a filter's walk knows nothing of its neighbours'
        e[m] = kofft::frontend_filter_walk(ints.data(), w.data(), x.data(), (int)num_mel, (int)m);
    return e;
}

static void same(const std::vector<uint64_t> &bins, const std::vector<float> &x)
{
    const std::vector<float> a = two_loops(bins, x), b = walks(bins, x);
    if (a.size() != b.size() || (a.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0)) ++bad;
}

int main()
{
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    std::mt19937_64 rng(54321);
    std::uniform_real_distribution<float> val(-1.0f, 2.0f);
    auto row = [&](size_t n) {
        std::vector<float> x(n);
        for (float &v : x) v = val(rng);
        if (n > 3) x[n / 2] = -0.0f, x[1] = 1e-41f;
        return x;
    };
    for (float rate : {16000.0f, 8000.0f, 22050.0f})
        for (size_t n_fft : {size_t(0), size_t(1), size_t(8), size_t(33), size_t(512)})
            for (size_t filters : {size_t(0), size_t(1), size_t(8), size_t(40), size_t(128)}) {
                std::vector<uint64_t> bins(filters + 2, 7);
                kofft_tables::mel_bins_f32(rate, n_fft, filters, bins.data());
                same(bins, row(n_fft));
            }
    same({0, 0}, row(0));
    same({0, 0}, row(5));
    same({3, 9}, row(5));
    same({0, 0, 0}, row(0));
    same({4, 4, 4, 4, 4}, row(16));
    same({0, 0, 0, top, top}, row(16));
    same({top, top, top}, row(16));
    same({0, 8, 16}, row(16));
    same({0, 8, top}, row(16));
    same({2, 5, 5, 9, 12, 40}, row(16));
    same({2, 5, 9, 9, 12, 16}, row(16));
    same({20, 30, 40, 50}, row(16));
    same({0, 1, 2, 3, (uint64_t(1) << 24) + 1, (uint64_t(1) << 40) + 3}, row(7));
    {
        std::vector<uint64_t> per_bin(34);
        for (size_t i = 0; i < per_bin.size(); ++i) per_bin[i] = i;
        same(per_bin, row(32));
    }
    for (int t = 0; t < 300; ++t) {
        const size_t n = rng() % 70, num_mel = rng() % 12;
        std::vector<uint64_t> bins(num_mel + 2);
        uint64_t at = rng() % 4;
        for (auto &b : bins) {
            const unsigned pick = rng() % 8;
            at += pick < 3 ? 0 : (pick == 7 ? rng() % 60 : rng() % 9);
            b = at;
        }
        if (t % 25 == 0) bins.back() = top;
        same(bins, row(n));
    }
    std::printf("sanitize_frontend_walk: %d problems\n", bad);
    return bad ? 1 : 0;
}
