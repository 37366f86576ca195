// sanitize_welch_cut.cpp -- kofft_amd/csrc/welch_cut.h against an enumeration of every frame, in a stand-alone program that
// tests/test_welch_cpu.py builds with -fsanitize=address,undefined.  For hand-made shapes and a few hundred random (frames per row,
// rows, cap): the chunks welch_chunk_end cuts cover every frame of the flat index exactly once in order, each holds at most
// max(cap, 32) frames, each begins and ends at a group seam, its pieces (frame_cut) are at most three rectangles that name every
// frame of the chunk once, every piece is made of whole groups, and welch_group_at counts the groups the chunk holds.
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/welch_cut.h"

using namespace kofft::host;

static long problems = 0, chunks = 0;

static bool seam(size_t t, size_t frames, size_t total)
{
    if (t == total) return true;
    const size_t f = t % frames;
    return f % kWelchGroup == 0;
}

static void walk(size_t frames, size_t rows, size_t cap)
{
    const size_t total = rows * frames, ngroups = welch_groups(frames);
    std::vector<int> seen(total, 0);
    size_t groups = 0;
    for (size_t t0 = 0; t0 < total;) {
        const size_t end = welch_chunk_end(t0, cap, frames, total);
        ++chunks;
        if (end <= t0 || end > total) {
            ++problems;
            return;
        }
        const size_t nt = end - t0;
        if (nt > (cap > kWelchGroup ? cap : kWelchGroup)) ++problems;
        if (!seam(t0, frames, total) || !seam(end, frames, total)) ++problems;
        const size_t g0 = welch_group_at(t0, frames), g1 = end == total ? rows * ngroups : welch_group_at(end, frames);
        if (g0 != groups || g1 <= g0) ++problems;
        groups = g1;
        FramePiece p[3];
        const int n = frame_cut(t0, nt, frames, p);
        if (n < 1 || n > 3) {
            ++problems;
            return;
        }
        size_t piece_groups = 0;
        for (int k = 0; k < n; ++k) {
            if (p[k].nr == 0 || p[k].nf == 0 || p[k].f0 + p[k].nf > frames || p[k].row + p[k].nr > rows || p[k].at + p[k].nr * p[k].nf > nt) {
                ++problems;
                continue;
            }
            // whole groups: the piece begins at a group's first frame and ends with a group (or the row)
            if (p[k].f0 % kWelchGroup != 0 || ((p[k].f0 + p[k].nf) % kWelchGroup != 0 && p[k].f0 + p[k].nf != frames)) ++problems;
            piece_groups += p[k].nr * (welch_groups(p[k].f0 + p[k].nf) - p[k].f0 / kWelchGroup);
            for (size_t j = 0; j < p[k].nr; ++j)
                for (size_t f = 0; f < p[k].nf; ++f) {
                    const size_t t = (p[k].row + j) * frames + p[k].f0 + f;
                    if (t < t0 || t >= end || t - t0 != p[k].at + j * p[k].nf + f) ++problems;
                    else ++seen[t];
                }
        }
        if (piece_groups != g1 - g0) ++problems;
        t0 = end;
    }
    if (groups != rows * ngroups) ++problems;
    for (size_t t = 0; t < total; ++t)
        if (seen[t] != 1) ++problems;
}

int main()
{
    // hand-made: one group, a seam inside a row, rows shorter than a group, caps below a group, the chunk test's shape (5 x 700)
    const size_t hand[][3] = {{1, 1, 1},   {31, 3, 40},  {32, 3, 32},   {33, 3, 33},    {65, 3, 64},  {65, 3, 70},   {65, 3, 1},
                              {700, 5, 508}, {700, 5, 254}, {700, 5, 3500}, {700, 5, 10000}, {7, 50, 100}, {64, 4, 96}, {100, 2, 31}};
    for (const auto &h : hand) walk(h[0], h[1], h[2]);
    {   // 5 rows x 700 frames, 508 frames per chunk: 480 | 220 + 288 (the end of row 0 and nine groups of row 1) | ...
        if (welch_chunk_end(0, 508, 700, 3500) != 480) ++problems;
        if (welch_chunk_end(480, 508, 700, 3500) != 700 + 288) ++problems;
        if (welch_group_at(480, 700) != 15 || welch_group_at(700, 700) != 22 || welch_groups(700) != 22) ++problems;
        if (welch_chunk_end(0, 5, 700, 3500) != 32 || welch_chunk_end(672, 5, 700, 3500) != 700) ++problems;
    }
    unsigned long long s = 0x9e3779b97f4a7c15ULL;  // xorshift: the same cases on every run
    auto rnd = [&](size_t m) {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (size_t)(s % m);
    };
    for (int i = 0; i < 400; ++i) {
        const size_t frames = 1 + rnd(i % 4 == 0 ? 40 : 300), rows = 1 + rnd(6), cap = 1 + rnd(i % 3 == 0 ? 64 : 2 * frames * rows);
        walk(frames, rows, cap);
    }
    std::printf("%ld chunks, %ld problems\n", chunks, problems);
    return problems ? 1 : 0;
}
