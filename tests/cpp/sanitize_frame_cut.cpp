// sanitize_frame_cut.cpp -- kofft_amd/csrc/frame_cut.h and the chunk walk and overlap test of kofft_amd/csrc/host_layout.h against
// enumerations, in a stand-alone program that tests/test_picture_cpu.py builds with -fsanitize=address,undefined.
//  * for every (frames per row, rows, chunk size) of a small grid, the chunks for_chunks hands out are consecutive, non-empty and
//    cover [0, total) exactly once; for every such chunk [t0, t0 + nt) of the flat index, the pieces are at most three, lie inside
//    the chunk's scratch, and together name every (row, frame) of the chunk exactly once, at the chunk position the flat order gives it;
//  * overlaps agrees with a byte-by-byte enumeration for every pair of ranges inside a 16-byte arena, empty and null ranges included;
//  * rows_span is the enumerated last element + 1 of a strided batch.
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/frame_cut.h"
#include "../../kofft_amd/csrc/host_layout.h"

using kofft::host::for_chunks;
using kofft::host::frame_cut;
using kofft::host::FramePiece;
using kofft::host::overlaps;
using kofft::host::rows_span;

int main()
{
    long problems = 0, chunks = 0;
    for (size_t frames = 1; frames <= 9; ++frames)
        for (size_t rows = 1; rows <= 5; ++rows)
            for (size_t chunk = 1; chunk <= rows * frames + 1; ++chunk) {
                const size_t total = rows * frames;
                size_t next = 0;  // where the next chunk has to begin
                const int walked = for_chunks(total, chunk, [&](size_t t0, size_t nt) {
                    if (t0 != next || nt == 0 || nt > chunk || t0 + nt > total) ++problems;
                    next = t0 + nt;
                    FramePiece p[3];
                    const int n = frame_cut(t0, nt, frames, p);
                    ++chunks;
                    if (n < 1 || n > 3) {
                        ++problems;
                        return 0;
                    }
                    std::vector<int> seen(nt, 0);
                    for (int k = 0; k < n; ++k) {
                        if (p[k].nr == 0 || p[k].nf == 0 || p[k].f0 + p[k].nf > frames || p[k].row + p[k].nr > rows ||
                            (p[k].nr > 1 && (p[k].f0 != 0 || p[k].nf != frames)) || p[k].at + p[k].nr * p[k].nf > nt) {
                            ++problems;
                            continue;
                        }
                        for (size_t j = 0; j < p[k].nr; ++j)
                            for (size_t f = 0; f < p[k].nf; ++f) {
                                const size_t t = (p[k].row + j) * frames + p[k].f0 + f;  // the flat index this piece element names
                                const size_t at = p[k].at + j * p[k].nf + f;             // where the piece puts it in the chunk
                                if (t < t0 || t - t0 != at) ++problems;
                                else ++seen[at];
                            }
                    }
                    for (size_t i = 0; i < nt; ++i)
                        if (seen[i] != 1) ++problems;
                    return 0;
                });
                if (walked != 0 || next != total) ++problems;
            }
    // the walk ends at the first body that fails and hands its code on; nothing to walk: no call
    {
        int calls = 0;
        if (for_chunks(10, 3, [&](size_t t0, size_t) { return ++calls, t0 == 3 ? 7 : 0; }) != 7 || calls != 2) ++problems;
        if (for_chunks(0, 0, [&](size_t, size_t) { return ++calls, 1; }) != 0 || calls != 2) ++problems;
    }
    // the seam test's shape (tests/test_gpu_picture.py): 3 rows x 601 frames, 512 per chunk
    {
        FramePiece p[3];
        const size_t want[4][3] = {{0, 0, 512}, {0, 512, 89}, {1, 0, 423}, {1, 423, 178}};
        int n = frame_cut(0, 512, 601, p);
        if (n != 1 || p[0].row != want[0][0] || p[0].f0 != want[0][1] || p[0].nf != want[0][2]) ++problems;
        n = frame_cut(512, 512, 601, p);
        if (n != 2 || p[0].row != want[1][0] || p[0].f0 != want[1][1] || p[0].nf != want[1][2] || p[1].row != want[2][0] ||
            p[1].f0 != want[2][1] || p[1].nf != want[2][2] || p[1].at != 89)
            ++problems;
        n = frame_cut(1024, 512, 601, p);
        if (n != 2 || p[0].row != want[3][0] || p[0].f0 != want[3][1] || p[0].nf != want[3][2] || p[1].row != 2 || p[1].nf != 334) ++problems;
        n = frame_cut(0, 1803, 601, p);
        if (n != 1 || p[0].nr != 3) ++problems;
    }
    // overlaps: every pair of ranges [a, a + na), [b, b + nb) inside a 16-byte arena against the bytes they share; a null range never
    long pairs = 0;
    {
        char arena[16] = {};
        for (size_t a = 0; a <= 16; ++a)
            for (size_t na = 0; a + na <= 16; ++na)
                for (size_t b = 0; b <= 16; ++b)
                    for (size_t nb = 0; b + nb <= 16; ++nb) {
                        bool shared = false;
                        for (size_t i = a; i < a + na; ++i) shared = shared || (i >= b && i < b + nb);
                        if (overlaps(arena + a, na, arena + b, nb) != shared) ++problems;
                        if (overlaps(nullptr, na, arena + b, nb) || overlaps(arena + a, na, nullptr, nb) || overlaps(nullptr, na, nullptr, nb))
                            ++problems;
                        ++pairs;
                    }
    }
    // rows_span: the last element + 1 that rows of len elements, row_stride apart, reach
    for (size_t rows = 0; rows <= 4; ++rows)
        for (size_t len = 0; len <= 5; ++len)
            for (size_t stride = len; stride <= len + 2; ++stride) {
                size_t last = 0;
                for (size_t r = 0; r < rows; ++r)
                    for (size_t i = 0; i < len; ++i) last = r * stride + i + 1 > last ? r * stride + i + 1 : last;
                if (rows_span(rows, len, stride) != last) ++problems;
                if (rows == 1 && rows_span(rows, len, 1000) != len) ++problems;  // one row: the stride does not count
            }
    std::printf("%ld chunks, %ld pairs of ranges, %ld problems\n", chunks, pairs, problems);
    return problems ? 1 : 0;
}
