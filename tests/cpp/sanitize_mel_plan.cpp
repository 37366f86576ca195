// sanitize_mel_plan.cpp -- the host side of the mel filterbank (kofft_amd/csrc/tables.cpp: mel_bins_f32, mel_plan_build) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, into exactly-sized buffers (ASan guards the ends): empty, all-equal,
// saturated and beyond-the-row edges, and random edge sets on which the plan, walked the way the kernels walk it (one ascending sweep,
// two accumulators), must give the bits of the reference's two loops per filter (cepstrum.rs:51-67).  Built and run by
// tests/test_mel_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

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

static std::vector<float> sweep(const std::vector<uint64_t> &bins, const std::vector<float> &x)
{
    const size_t num_mel = bins.size() - 2, n = x.size();
    std::vector<int> ints(kofft_tables::mel_plan_ints(num_mel));
    std::vector<float> w(2 * n);
    kofft_tables::mel_plan_build(bins.data(), n, num_mel, ints.data(), w.data());
    const int *seg = ints.data(), *live = ints.data() + 2 * (num_mel + 1);
    std::vector<float> e(num_mel, 0.0f);
    float rise = 0.0f, fall = 0.0f;
    for (size_t s = 0; s <= num_mel; ++s) {
        if (seg[2 * s] < 0 || seg[2 * s] > seg[2 * s + 1] || (size_t)seg[2 * s + 1] > n) ++bad;
        if (s && seg[2 * s] != seg[2 * s - 1]) ++bad;  // the clamped segments tile [seg[0], seg[2 num_mel + 1])
        for (int k = seg[2 * s]; k < seg[2 * s + 1]; ++k) {
            rise = rise + w[2 * k] * x[k];
            fall = fall + w[2 * k + 1] * x[k];
        }
        if (s >= 1) e[s - 1] = live[s - 1] ? fall : 0.0f;
        fall = rise;
        rise = 0.0f;
    }
    return e;
}

static void same(const std::vector<uint64_t> &bins, const std::vector<float> &x)
{
    const std::vector<float> a = two_loops(bins, x), b = sweep(bins, x);
    if (a.size() != b.size() || (a.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0)) ++bad;
}

int main()
{
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<float> val(0.0f, 2.0f);
    auto row = [&](size_t n) {
        std::vector<float> x(n);
        for (float &v : x) v = val(rng);
        return x;
    };
    // the edge helper: reference settings, no filters, rates that make every point NaN, negative or infinite (the saturating cast)
    const float rates[] = {16000.0f, 8000.0f, 0.0f, -16000.0f, 1e-30f, 3e38f, std::numeric_limits<float>::quiet_NaN(),
                           std::numeric_limits<float>::infinity()};
    for (float rate : rates)
        for (size_t n_fft : {size_t(0), size_t(1), size_t(8), size_t(33), size_t(512), size_t(1) << 24})
            for (size_t filters : {size_t(0), size_t(1), size_t(8), size_t(40), size_t(4096)}) {
                std::vector<uint64_t> bins(filters + 2, 7);
                kofft_tables::mel_bins_f32(rate, n_fft, filters, bins.data());
                if (rate == 16000.0f || rate == 8000.0f) {
                    if (bins[0] != 0) ++bad;
                    for (size_t i = 0; i + 1 < bins.size(); ++i)
                        if (bins[i + 1] < bins[i]) ++bad;
                    if (n_fft <= 512) same(bins, row(n_fft));
                }
            }
    // hand-made edges: empty, all equal, saturated, beyond the row, a dead filter between two live ones, one filter over the row
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
    // random nondecreasing edge sets with repeats and edges past the row
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
    std::printf("sanitize_mel_plan: %d problems\n", bad);
    return bad ? 1 : 0;
}
