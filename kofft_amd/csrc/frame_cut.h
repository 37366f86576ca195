// frame_cut.h -- a chunk [t0, t0 + nt) of the flat frame index t = row * frames + frame, cut into at most three rectangles of the
// batch: the rest of its first row, whole rows, and the head of its last row.  The rows kernels have no starting index, so every
// framed family that produces (k_stft_rows.hip: framed_produce) or renders (k_picture_f32.hip) a chunk by launches of them cuts it
// here.  Arithmetic only, no HIP: tests/cpp/sanitize_frame_cut.cpp includes this file alone and compares it with an enumeration of
// every frame.
#pragma once
#include <cstddef>

namespace kofft {
namespace host {

// frames [f0, f0 + nf) of each of the rows [row, row + nr); nr > 1: f0 == 0 and nf == frames.  The piece's first frame is frame `at`
// of the chunk, and its frames follow densely, row after row.
struct FramePiece {
    size_t row, nr, f0, nf, at;
};

// returns the number of pieces (0 .. 3); frames >= 1, t0 + nt <= rows * frames
inline int frame_cut(size_t t0, size_t nt, size_t frames, FramePiece *p)
{
    int n = 0;
    const size_t end = t0 + nt;
    for (size_t t = t0; t < end;) {
        const size_t r = t / frames, f = t - r * frames;
        size_t done;
        if (f != 0 || end - t < frames) {  // part of row r
            done = frames - f < end - t ? frames - f : end - t;
            p[n++] = FramePiece{r, 1, f, done, t - t0};
        } else {
            const size_t nr = (end - t) / frames;
            done = nr * frames;
            p[n++] = FramePiece{r, nr, 0, frames, t - t0};
        }
        t += done;
    }
    return n;
}

}  // namespace host
}  // namespace kofft
