// welch_cut.h -- the chunks of the composed Welch / cross-spectrum route.  The frames of `rows` rows carry the flat index
// t = row * frames + frame; every row is cut into groups of KOFFT_HIP_WELCH_GROUP consecutive frames counted from its frame 0 (the last
// one shorter), and a group's partial sum must be formed in one piece.  A chunk [t0, end) of at most `cap` frames therefore begins and
// ends at a group seam: welch_chunk_end cuts it, frame_cut (frame_cut.h) cuts the chunk into rectangles of the batch, and the
// rectangles are whole groups because the chunk is.  Arithmetic only, no HIP: tests/cpp/sanitize_welch_cut.cpp includes this file
// alone and compares it with an enumeration of every frame.
#pragma once
#include <cstddef>

#include "frame_cut.h"

#ifndef KOFFT_HIP_WELCH_GROUP
#define KOFFT_HIP_WELCH_GROUP 32
#endif

namespace kofft {
namespace host {

constexpr size_t kWelchGroup = KOFFT_HIP_WELCH_GROUP;

// groups of one row of `frames` frames
inline size_t welch_groups(size_t frames) { return frames / kWelchGroup + (frames % kWelchGroup != 0); }

// The end of the chunk that begins at t0, a group seam (t0 < total = rows * frames, frames >= 1): the last seam at or before t0 + cap,
// or, where not even t0's own group fits `cap` frames, the end of that group (a group is never split, so the scratch of a chunk holds
// max(cap, kWelchGroup) frames).
inline size_t welch_chunk_end(size_t t0, size_t cap, size_t frames, size_t total)
{
    if (total - t0 <= cap) return total;
    const size_t e = t0 + cap, r = e / frames, f = e - r * frames;
    const size_t seam = r * frames + f / kWelchGroup * kWelchGroup;  // (f == 0: the end of row r - 1, a seam too)
    if (seam > t0) return seam;
    const size_t r0 = t0 / frames, f0 = t0 - r0 * frames;
    return r0 * frames + (frames - f0 < kWelchGroup ? frames : f0 + kWelchGroup);
}

// the flat group index row * welch_groups(frames) + group of the group that begins at frame t (a seam), or of the end of the batch
inline size_t welch_group_at(size_t t, size_t frames)
{
    const size_t r = t / frames, f = t - r * frames;
    return r * welch_groups(frames) + f / kWelchGroup;
}

}  // namespace host
}  // namespace kofft
