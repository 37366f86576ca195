// sanitize_picture_cut.cpp -- kofft_amd/csrc/picture_cut.h against an enumeration of every frame, in a stand-alone program that
// tests/test_picture_cpu.py builds with -fsanitize=address,undefined: for every (frames per row, rows, chunk size) of a small grid and
// every chunk [t0, t0 + nt) of the flat index, the pieces are at most three, lie inside the chunk's scratch, and together name every
// (row, frame) of the chunk exactly once, at the chunk position the flat order gives it.
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/picture_cut.h"

using kofft::host::PicPiece;
using kofft::host::picture_cut;

int main()
{
    long problems = 0, chunks = 0;
    for (size_t frames = 1; frames <= 9; ++frames)
        for (size_t rows = 1; rows <= 5; ++rows)
            for (size_t chunk = 1; chunk <= rows * frames + 1; ++chunk) {
                const size_t total = rows * frames;
                for (size_t t0 = 0; t0 < total; t0 += chunk) {
                    const size_t nt = total - t0 < chunk ? total - t0 : chunk;
                    PicPiece p[3];
                    const int n = picture_cut(t0, nt, frames, p);
                    ++chunks;
                    if (n < 1 || n > 3) {
                        ++problems;
                        continue;
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
                }
            }
    // the seam test's shape (tests/test_gpu_picture.py): 3 rows x 601 frames, 512 per chunk
    {
        PicPiece p[3];
        const size_t want[4][3] = {{0, 0, 512}, {0, 512, 89}, {1, 0, 423}, {1, 423, 178}};
        int n = picture_cut(0, 512, 601, p);
        if (n != 1 || p[0].row != want[0][0] || p[0].f0 != want[0][1] || p[0].nf != want[0][2]) ++problems;
        n = picture_cut(512, 512, 601, p);
        if (n != 2 || p[0].row != want[1][0] || p[0].f0 != want[1][1] || p[0].nf != want[1][2] || p[1].row != want[2][0] ||
            p[1].f0 != want[2][1] || p[1].nf != want[2][2] || p[1].at != 89)
            ++problems;
        n = picture_cut(1024, 512, 601, p);
        if (n != 2 || p[0].row != want[3][0] || p[0].f0 != want[3][1] || p[0].nf != want[3][2] || p[1].row != 2 || p[1].nf != 334) ++problems;
        n = picture_cut(0, 1803, 601, p);
        if (n != 1 || p[0].nr != 3) ++problems;
    }
    std::printf("%ld chunks, %ld problems\n", chunks, problems);
    return problems ? 1 : 0;
}
