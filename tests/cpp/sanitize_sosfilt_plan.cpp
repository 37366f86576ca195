// sosfilt_plan.h (the index arithmetic of the batched IIR filter) against an enumeration, stand-alone and meant to be
// built with -fsanitize=address,undefined: for small rows, nx and T, both directions, the tiled kernel's walk -- row groups, tiles in
// their order, the samples of a tile in their order -- visits every sample of every row exactly once, in ascending (descending) time,
// and the wavefront's copies of a tile (sos_tile_elem over k = lane + 64 j) touch exactly the elements that exist, each once, inside
// an LDS image of 64 rows of sos_lds_stride(T) floats.  Then the passes of a cascade.  Prints "... 0 problems" and exits 0 when all hold.
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/sosfilt_plan.h"

using namespace kofft::host;

static long g_problems = 0, g_checks = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        ++g_checks;                                                                     \
        if (!(cond) && ++g_problems <= 20) std::printf("PROBLEM line %d: %s\n", __LINE__, #cond); \
    } while (0)

static void walk(unsigned long long rows, unsigned long long nx, unsigned T, bool reverse)
{
    std::vector<int> seen(rows * nx, 0);       // the caller's buffer: every index into it is checked by the sanitizer
    std::vector<long long> last(rows, reverse ? (long long)nx : -1);
    const unsigned S = sos_lds_stride(T);
    CHECK(S % 2 == 1 && S >= T);
    const unsigned long long ngroups = sos_row_groups(rows), ntiles = sos_tiles(nx, T);
    CHECK((ngroups - 1) * kSosRows < rows && ngroups * kSosRows >= rows);
    CHECK((ntiles - 1) * T < nx && ntiles * T >= nx);
    unsigned long long rows_seen = 0;
    for (unsigned long long g = 0; g < ngroups; ++g) {
        const unsigned nrows = sos_group_rows(g, rows);
        CHECK(nrows >= 1 && nrows <= kSosRows);
        rows_seen += nrows;
        std::vector<int> tiles_seen(ntiles, 0);
        for (unsigned long long step = 0; step < ntiles; ++step) {
            const unsigned long long tl = sos_tile_at(step, ntiles, reverse);
            CHECK(tl < ntiles);
            if (tl >= ntiles) continue;
            ++tiles_seen[tl];
            const unsigned len = sos_tile_len(tl, nx, T);
            CHECK(len >= 1 && len <= T && tl * T + len <= nx);
            // the copies: 64 lanes, R * T / 64 elements each
            std::vector<int> lds(kSosRows * S, 0);
            unsigned touched = 0;
            for (unsigned j = 0; j < kSosRows * T / 64; ++j)
                for (unsigned lane = 0; lane < 64; ++lane) {
                    unsigned r, t;
                    sos_tile_elem(lane + 64 * j, T, &r, &t);
                    CHECK(r < kSosRows && t < T);
                    unsigned r0, t0;
                    sos_tile_elem(lane, T, &r0, &t0);
                    CHECK(r == r0 + (64 / T) * j && t == t0);  // (the kernel's form of the same element)
                    ++lds[r * S + t];
                    if (r < nrows && t < len) {
                        ++seen[(g * kSosRows + r) * nx + tl * T + t];  // the global element this lane fetches and stores
                        ++touched;
                    }
                }
            CHECK(touched == nrows * len);
            for (unsigned r = 0; r < kSosRows; ++r)
                for (unsigned t = 0; t < S; ++t) CHECK(lds[r * S + t] == (t < T ? 1 : 0));
            // the walk of every row of the group
            for (unsigned r = 0; r < nrows; ++r)
                for (unsigned i = 0; i < len; ++i) {
                    const unsigned long long t = sos_walk_at(i, len, reverse);
                    CHECK(t < len);
                    const long long at = (long long)(tl * T + t);
                    CHECK(reverse ? at == last[g * kSosRows + r] - 1 : at == last[g * kSosRows + r] + 1);
                    last[g * kSosRows + r] = at;
                }
        }
        for (unsigned long long tl = 0; tl < ntiles; ++tl) CHECK(tiles_seen[tl] == 1);
    }
    CHECK(rows_seen == rows);
    for (unsigned long long k = 0; k < rows * nx; ++k) CHECK(seen[k] == 1);
    for (unsigned long long r = 0; r < rows; ++r) CHECK(last[r] == (reverse ? 0 : (long long)nx - 1));
    // the plain kernel's walk of a whole row
    long long prev = reverse ? (long long)nx : -1;
    for (unsigned long long i = 0; i < nx; ++i) {
        const long long t = (long long)sos_walk_at(i, nx, reverse);
        CHECK(reverse ? t == prev - 1 : t == prev + 1);
        prev = t;
    }
}

int main()
{
    const unsigned long long row_counts[] = {1, 2, 63, 64, 65, 130};
    const unsigned tiles[] = {16, 32, 64};
    for (unsigned T : tiles)
        for (unsigned long long rows : row_counts)
            for (unsigned long long nx = 1; nx <= 3 * T + 2; nx += (nx < 4 || nx + 3 > T) ? 1 : 7)
                for (int reverse = 0; reverse < 2; ++reverse) walk(rows, nx, T, reverse != 0);
    CHECK(kSosTile == 16 || kSosTile == 32 || kSosTile == 64);
    for (unsigned G = 1; G <= 9; ++G)
        for (unsigned long long sections = 1; sections <= 40; ++sections) {
            const unsigned long long passes = sos_passes(sections, G);
            unsigned long long total = 0;
            for (unsigned long long p = 0; p < passes; ++p) {
                const unsigned ns = sos_pass_sections(p, sections, G);
                CHECK(ns >= 1 && ns <= G && p * G == total);
                total += ns;
            }
            CHECK(total == sections);
        }
    // the largest sizes: no overflow in the counts
    CHECK(sos_tiles(~0ull, 32) == (1ull << 59) && sos_row_groups(~0ull) == (1ull << 58) && sos_passes(~0ull, 8) == (1ull << 61));
    CHECK(sos_tile_len((1ull << 59) - 1, ~0ull, 32) == 31 && sos_group_rows((1ull << 58) - 1, ~0ull) == 63);
    std::printf("%ld checks, %ld problems\n", g_checks, g_problems);
    return g_problems ? 1 : 0;
}
