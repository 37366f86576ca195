// sanitize_resample_plan.cpp -- kofft_amd/csrc/resample_plan.h against an enumeration of every term, in a stand-alone program that
// tests/test_resample_cpu.py builds with -fsanitize=address,undefined.  For every up, down, nh up to 12, a few nx, t0 and tile sizes:
// the phase and sample of every output of every tile, the terms per phase, the range of terms that exist, the samples a tile stages
// (every term its outputs name lies inside them, at the place the kernel reads), the LDS footprint that holds them, and the route
// query's monotony in nh.
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/resample_plan.h"

using namespace kofft::host;
typedef unsigned long long u64;

static long problems = 0, tiles = 0, outputs = 0;
#define EXPECT(c)                                                                       \
    do {                                                                                \
        if (!(c)) {                                                                     \
            if (++problems <= 10) std::printf("line %d: %s\n", __LINE__, #c);           \
        }                                                                               \
    } while (0)

static void walk(u64 up, u64 down, u64 nh, u64 nx, u64 t0, u64 tile)
{
    const u64 full_up = (nx - 1) * up + nh;
    if (t0 >= full_up) return;
    const u64 out_len = (full_up - t0 - 1) / down + 1;  // every output that begins inside the full result
    const u64 J = resample_max_terms(nh, up), stride = resample_tap_stride(J), span = resample_tile_span(up, down, tile);
    const u64 words = resample_lds_words(nh, up, down, tile);
    EXPECT(stride >= J && stride % 2 == 1 && words == up * stride + span + J);
    {   // J by enumeration
        u64 j = 0;
        while (j * up < nh) ++j;
        EXPECT(j == J);
    }
    for (u64 w : {1, 2, 3, 4}) {  // a thread's outputs dm, dm + w, ..: one phase, samples w * down / up apart, where the plan says so
        bool same = true;
        for (unsigned r = 0; r < up; ++r)
            for (unsigned dm = 0; dm < 8; ++dm) {
                unsigned p0 = 0, d0 = 0, p1 = 0, d1 = 0;
                resample_output(r, dm, (unsigned)up, (unsigned)down, &p0, &d0);
                resample_output(r, dm + (unsigned)w, (unsigned)up, (unsigned)down, &p1, &d1);
                if (p0 != p1 || (d1 - d0) * up != w * down) same = false;
            }
        EXPECT(same == resample_same_phase(up, down, w));
    }
    {   // the lanes of the shared-phase instance: a multiple of the phases' period, at least three quarters of the workgroup
        const unsigned lanes = resample_phase_lanes(up, down), outs = resample_tile_outputs(up, down);
        EXPECT(lanes <= kResampleThreads && (lanes == 0 || (lanes >= 192 && resample_same_phase(up, down, lanes))));
        EXPECT(outs == (lanes ? 4 * lanes : kResampleTile) && outs <= kResampleTile);
        if (lanes == 0)
            for (u64 w = 192; w <= kResampleThreads; ++w) EXPECT(!resample_same_phase(up, down, w));
        else
            for (u64 w = lanes + 1; w <= kResampleThreads; ++w) EXPECT(!resample_same_phase(up, down, w));
    }
    for (u64 m0 = 0; m0 < out_len; m0 += tile) {
        const u64 n = out_len - m0 < tile ? out_len - m0 : tile;
        const ResampleTile tl = resample_tile(t0, m0, n, up, down, J);
        ++tiles;
        EXPECT(tl.s_count <= span + J);
        std::vector<float> staged(tl.s_count, 0.0f);  // the kernel's LDS run: an index outside it is the sanitizer's to report
        std::vector<float> table(up * stride, 0.0f);
        for (u64 dm = 0; dm < n; ++dm) {
            ++outputs;
            const u64 t = t0 + (m0 + dm) * down, p = t % up, i0 = t / up;
            unsigned gp = 0, gdi = 0;
            resample_output(tl.r_first, (unsigned)dm, (unsigned)up, (unsigned)down, &gp, &gdi);
            EXPECT(gp == p && tl.q_first + gdi == i0);
            u64 cnt = 0;
            while (p + cnt * up < nh) ++cnt;
            EXPECT(resample_terms<u64>(nh, up, p) == cnt);
            EXPECT(resample_terms<unsigned>((unsigned)nh, (unsigned)up, (unsigned)p) == cnt);
            u64 jlo = 0, jhi = 0;
            resample_term_range(i0, nx, cnt, &jlo, &jhi);
            EXPECT(jlo <= jhi && jhi <= cnt);
            for (u64 j = 0; j < cnt; ++j) {
                const bool live = i0 >= j && i0 - j < nx;
                EXPECT(live == (j >= jlo && j < jhi));
                // the place of term j in the staged run and in the tap table
                const long long sample = (long long)i0 - (long long)j;
                const long long at = (long long)gdi + (long long)(J - 1) - (long long)j;
                EXPECT(at >= 0 && (u64)at < tl.s_count && tl.s_first + at == sample);
                if (at >= 0 && (u64)at < tl.s_count) staged[(size_t)at] += 1.0f;
                table[p * stride + j] += 1.0f;
            }
        }
        // the first output's oldest named sample is the run's first, the last output's newest its last
        EXPECT(tl.s_first == (long long)((t0 + m0 * down) / up) - (long long)(J - 1));
        EXPECT(tl.s_first + (long long)tl.s_count - 1 == (long long)((t0 + (m0 + n - 1) * down) / up));
    }
}

int main()
{
    for (u64 up = 1; up <= 12; ++up)
        for (u64 down = 1; down <= 12; ++down)
            for (u64 nh = 1; nh <= 12; ++nh)
                for (u64 nx : {1, 2, 3, 7, 12})
                    for (u64 t0 : {0, 1, 5, 11, 40})
                        for (u64 tile : {1, 3, 8}) walk(up, down, nh, nx, t0, tile);
    walk(160, 441, 8821, 50, 4410, 64);
    walk(441, 160, 1765, 20, 3, 1024);
    EXPECT(resample_phase_lanes(1, 3) == 256 && resample_phase_lanes(3, 1) == 255 && resample_phase_lanes(4, 2) == 256 &&
           resample_phase_lanes(160, 441) == 0 && resample_phase_lanes(441, 160) == 0 && resample_phase_lanes(7, 5) == 252);
    // the route: 1 up to some nh and 0 beyond; a shape that fits keeps every 32-bit offset of the tiled kernel's walk below 2^32
    const u64 pairs[][2] = {{1, 1}, {3, 2}, {1, 3}, {160, 441}, {441, 160}, {4099, 1}, {1, 13}, {1, 14}, {13312, 1}, {13313, 1}};
    for (const auto &pr : pairs) {
        int before = 1;
        for (u64 nh = 1; nh <= 70000; nh += (nh < 300 ? 1 : 97)) {
            const int r = resample_route(nh, pr[0], pr[1]);
            EXPECT(r == 0 || r == 1);
            EXPECT(!(before == 0 && r == 1));
            before = r;
            if (resample_fits(nh, pr[0], pr[1])) {
                const u64 span = resample_tile_span(pr[0], pr[1], kResampleTile);
                EXPECT((span + 1) * pr[0] < (1ULL << 32) && nh < (1ULL << 32));
                EXPECT(resample_lds_words(nh, pr[0], pr[1], kResampleTile) * 4 <= 64 * 1024);
            } else {
                EXPECT(r == 0);
            }
        }
    }
    EXPECT(resample_route(61, 1, 3) == 1 && resample_route(1, ~0ULL, 1) == 0 && resample_route(~0ULL, 1, 1) == 0 &&
           resample_route(5, 1, ~0ULL) == 0);
    std::printf("%ld tiles, %ld outputs, %ld problems\n", tiles, outputs, problems);
    return problems ? 1 : 0;
}
