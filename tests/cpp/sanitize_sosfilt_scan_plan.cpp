// The scan functions of sosfilt_plan.h against an enumeration, stand-alone and meant to be built with
// -fsanitize=address,undefined: for small batches, both directions, both walks of the scan -- the wavefronts of 64 virtual rows, the
// tiles of a chunk in their order, the copies of a tile as the kernel counts them -- visit every sample of every chunk exactly once, in
// ascending (descending) time inside a row, chunk c ending where chunk c + 1 begins, and never a sample outside the batch.  The first
// walk (per_row = C - 1) leaves exactly the last chunk of every row out.  Prints "... 0 problems" and exits 0 when all hold.
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

// store: the second walk (every chunk); otherwise the first one (every chunk but a row's last)
static void walk(unsigned long long rows, unsigned long long nx, unsigned long long chunk, bool reverse, bool store)
{
    const unsigned T = kSosTile;
    const unsigned long long C = sos_scan_chunks(nx, chunk);
    CHECK((C - 1) * chunk < nx && C * chunk >= nx);
    const unsigned long long per = store ? C : C - 1;
    std::vector<int> seen(rows * nx, 0);  // the caller's buffer: every index into it is checked by the sanitizer
    std::vector<long long> last(rows, reverse ? (long long)nx : -1);
    if (per == 0) return;
    const unsigned long long nv = rows * per, ngroups = sos_row_groups(nv);
    const unsigned long long span = nx < chunk ? nx : chunk, ntiles = sos_tiles(span, T);
    for (unsigned long long g = 0; g < ngroups; ++g) {
        const unsigned nvr = sos_group_rows(g, nv);
        CHECK(nvr >= 1 && nvr <= kSosRows);
        // the walk of every lane, tile by tile; a lane's chunk is walked in the order of its steps
        for (unsigned lane = 0; lane < nvr; ++lane) {
            unsigned long long row, c;
            sos_scan_vrow(g * kSosRows + lane, per, &row, &c);
            CHECK(row < rows && c < per);
            if (row >= rows || c >= per) continue;
            const unsigned long long len = sos_scan_len(c, nx, chunk);
            CHECK(len >= 1 && len <= chunk && c * chunk + len <= nx);
            CHECK(c + 1 == C || len == chunk);
            CHECK(store || len == chunk);
            unsigned long long walked = 0;
            for (unsigned long long k = 0; k < ntiles; ++k) {
                const unsigned tl = sos_scan_tile_len(len, k, T);
                CHECK(tl <= T && (tl == 0 ? k * T >= len : k * T + tl <= len) && (tl == T || k * T + tl >= len));
                for (unsigned t = 0; t < tl; ++t) {
                    const unsigned long long at = sos_scan_at(row, c, k * T + t, nx, chunk, reverse);
                    CHECK(at >= row * nx && at < (row + 1) * nx);
                    if (at < row * nx || at >= (row + 1) * nx) continue;
                    ++seen[at];
                    ++walked;
                    const long long s = (long long)(at - row * nx);
                    if (k == 0 && t == 0) {  // a chunk begins where the one before it ended
                        const long long first = reverse ? (long long)nx - 1 - (long long)(c * chunk) : (long long)(c * chunk);
                        CHECK(s == first);
                        last[row] = reverse ? s + 1 : s - 1;
                    }
                    CHECK(s == (reverse ? last[row] - 1 : last[row] + 1));
                    last[row] = s;
                }
            }
            CHECK(walked == len);  // ntiles covers the longest chunk
        }
        // the copies: element j of lane (r0, t0) is virtual row r0 + (64 / T) * j, step k * T + t0; it exists where that step < len
        for (unsigned long long k = 0; k < ntiles; ++k) {
            unsigned long long copied = 0, want = 0;
            for (unsigned lane = 0; lane < nvr; ++lane) {
                unsigned long long row, c;
                sos_scan_vrow(g * kSosRows + lane, per, &row, &c);
                want += sos_scan_tile_len(sos_scan_len(c, nx, chunk), k, T);
            }
            for (unsigned j = 0; j < T; ++j)
                for (unsigned lane = 0; lane < 64; ++lane) {
                    unsigned r0, t0;
                    sos_tile_elem(lane, T, &r0, &t0);
                    const unsigned r = r0 + (64 / T) * j;
                    CHECK(r < kSosRows && t0 < T);
                    if (r >= nvr) continue;
                    unsigned long long row, c;
                    sos_scan_vrow(g * kSosRows + r, per, &row, &c);
                    if (k * T + t0 < sos_scan_len(c, nx, chunk)) {
                        const unsigned long long at = sos_scan_at(row, c, k * T + t0, nx, chunk, reverse);
                        CHECK(at < rows * nx);
                        if (at < rows * nx) seen[at] += 16;
                        ++copied;
                    }
                }
            CHECK(copied == want);
        }
    }
    for (unsigned long long r = 0; r < rows; ++r)
        for (unsigned long long t = 0; t < nx; ++t) {
            const unsigned long long step = reverse ? nx - 1 - t : t;
            const bool walked = store || step < (C - 1) * chunk;
            CHECK(seen[r * nx + t] == (walked ? 17 : 0));  // once by the walk, once by the copies
        }
}

int main()
{
    const unsigned long long nxs[] = {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200, 43 * 32 - 7, 64 * 32 + 5, 130 * 32 + 1};
    for (unsigned long long chunk : {32ull, 64ull, 96ull, 4096ull, 1ull << 40})
        for (unsigned long long nx : nxs)
            for (unsigned long long rows : {1ull, 2ull, 3ull, 65ull})
                for (int reverse = 0; reverse < 2; ++reverse)
                    for (int store = 0; store < 2; ++store) walk(rows, nx, chunk, reverse != 0, store != 0);
    // the state scratch: a slot a seam, then D slots for the matrix
    CHECK(sos_scan_state_floats(3, 5, 16) == (3 * 4 + 16 + 3) * 16);
    for (unsigned long long row = 0; row < 3; ++row) {  // the Z_0 slots lie behind the seams and the matrix, inside the scratch
        CHECK(sos_scan_z0_slot(row, 3, 5, 16) == 3 * 4 + 16 + row);
        CHECK((sos_scan_z0_slot(row, 3, 5, 16) + 1) * 16 <= sos_scan_state_floats(3, 5, 16));
    }
    // the chunk rule: a multiple of the tile, never below the floor
    for (unsigned long long rows : {1ull, 2ull, 15ull, 16ull, 64ull, 4096ull, 65536ull})
        for (unsigned long long nx : {1ull, 3000ull, 1ull << 20, 28800000ull, 1ull << 24})
            for (unsigned long long sections : {1ull, 4ull, 8ull, 12ull}) {
                const unsigned long long k = sos_scan_chunk_rule(rows, nx, sections);
                CHECK(k >= kSosScanMinChunk && k % kSosTile == 0);
            }
    std::printf("sosfilt scan plan: %ld checks, %ld problems\n", g_checks, g_problems);
    return g_problems ? 1 : 0;
}
