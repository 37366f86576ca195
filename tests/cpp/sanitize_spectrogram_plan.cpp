// sanitize_spectrogram_plan.cpp -- the host side of the log-scaled spectrogram render (kofft_amd/csrc/tables.cpp: log_bin_map,
// spec_ranges_build) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, into exactly-sized buffers (ASan guards the
// ends): the reference-shaped table of every bins from 1 to 8192 must be nondecreasing with entries below bins, its ranges must tile
// [0, bins) and, walked the way the kernels walk them, give the bits of log_scale_bins' scatter loop (spectrogram.rs:220-234);
// tables with an entry >= bins or a decreasing step must be refused; random nondecreasing tables must round-trip.  Built and run by
// tests/test_spectrogram_oracle.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../kofft_amd/csrc/tables.h"

static int bad = 0;

// log_scale_bins over a table (spectrogram.rs:220-234)
static std::vector<float> scatter(const std::vector<uint32_t> &table, const std::vector<float> &x)
{
    const size_t bins = table.size();
    std::vector<float> accum(bins, 0.0f);
    std::vector<uint32_t> counts(bins, 0);
    for (size_t b = 0; b < bins; ++b) {
        accum[table[b]] += x[b];
        counts[table[b]] += 1;
    }
    for (size_t p = 0; p < bins; ++p)
        if (counts[p] > 0) accum[p] /= (float)counts[p];
    return accum;
}

// the kernels' walk: pixel p sums its range from +0 and divides once
static std::vector<float> ranges(const std::vector<uint32_t> &start, const std::vector<float> &x)
{
    const size_t bins = x.size();
    std::vector<float> out(bins, 0.0f);
    for (size_t p = 0; p < bins; ++p) {
        float sum = 0.0f;
        for (uint32_t k = start[p]; k < start[p + 1]; ++k) sum += x[k];
        if (start[p + 1] > start[p]) sum = sum / (float)(start[p + 1] - start[p]);
        out[p] = sum;
    }
    return out;
}

static void check_table(const std::vector<uint32_t> &table, std::mt19937 &rng, const char *what)
{
    const size_t bins = table.size();
    std::vector<uint32_t> start(bins + 1);
    if (!kofft_tables::spec_ranges_build(table.data(), bins, start.data())) {
        std::printf("%s bins=%zu: refused\n", what, bins);
        ++bad;
        return;
    }
    if (start[0] != 0 || start[bins] != bins) ++bad;
    for (size_t p = 0; p < bins; ++p) {
        if (start[p] > start[p + 1]) ++bad;
        for (uint32_t k = start[p]; k < start[p + 1]; ++k)
            if (table[k] != p) ++bad;
    }
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    std::vector<float> x(bins);
    for (auto &v : x) v = u(rng);
    if (bins > 2) x[bins / 2] = -0.0f;
    const std::vector<float> a = scatter(table, x), b = ranges(start, x);
    if (std::memcmp(a.data(), b.data(), bins * sizeof(float)) != 0) {
        std::printf("%s bins=%zu: the ranges and the scatter loop differ\n", what, bins);
        ++bad;
    }
}

int main()
{
    std::mt19937 rng(20261019);
    size_t most = 0;
    for (size_t bins = 1; bins <= 8192; ++bins) {
        std::vector<uint32_t> table(bins);
        kofft_tables::log_bin_map(bins, table.data());
        for (size_t b = 0; b < bins; ++b) {
            if (table[b] >= bins || (b && table[b] < table[b - 1])) {
                std::printf("log_bin_map(%zu): entry %zu\n", bins, b);
                ++bad;
            }
        }
        if (bins <= 600 || bins % 97 == 0 || bins == 8192) check_table(table, rng, "log_bin_map");
        if (bins == 8192) {
            std::vector<uint32_t> start(bins + 1);
            kofft_tables::spec_ranges_build(table.data(), bins, start.data());
            for (size_t p = 0; p < bins; ++p) most = std::max<size_t>(most, start[p + 1] - start[p]);
        }
    }
    std::printf("bins per pixel at 8192: at most %zu\n", most);
    {  // the case the issue keeps: at 16 bins the top pixel is 14
        std::vector<uint32_t> t(16);
        kofft_tables::log_bin_map(16, t.data());
        if (t[15] != 14 || t[0] != 0) ++bad;
        std::vector<uint32_t> one(1, 7);
        kofft_tables::log_bin_map(1, one.data());
        if (one[0] != 0) ++bad;
        kofft_tables::log_bin_map(0, nullptr);
    }
    // random nondecreasing tables, empty pixels and long ranges included
    for (int round = 0; round < 400; ++round) {
        const size_t bins = 1 + rng() % 300;
        std::vector<uint32_t> table(bins);
        uint32_t y = 0;
        for (size_t b = 0; b < bins; ++b) {
            if (rng() % 3 == 0) y += rng() % 4;
            if (y >= bins) y = (uint32_t)bins - 1;
            table[b] = y;
        }
        check_table(table, rng, "random");
    }
    // refusals: an entry >= bins, a decreasing step
    {
        std::vector<uint32_t> start(5);
        const uint32_t over[4] = {0, 1, 2, 4}, down[4] = {0, 2, 1, 3}, top[4] = {0, 0, 0, 0xffffffffu}, fine[4] = {3, 3, 3, 3};
        if (kofft_tables::spec_ranges_build(over, 4, start.data())) ++bad;
        if (kofft_tables::spec_ranges_build(down, 4, start.data())) ++bad;
        if (kofft_tables::spec_ranges_build(top, 4, start.data())) ++bad;
        if (!kofft_tables::spec_ranges_build(fine, 4, start.data())) ++bad;
        if (start[0] != 0 || start[3] != 0 || start[4] != 4) ++bad;
        std::vector<uint32_t> none(1);
        if (!kofft_tables::spec_ranges_build(nullptr, 0, none.data()) || none[0] != 0) ++bad;
    }
    std::printf("%d problems\n", bad);
    return bad ? 1 : 0;
}
