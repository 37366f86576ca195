// persist_walk.h -- which way a kClaim launch of the persistent kernel (fft_persist.hip.h, PersistClaim) walks its batch, and where its
// kept zone begins.  Arithmetic only, no HIP: tests/cpp/sanitize_persist_walk.cpp includes this file alone.
//
// The kernel hands out WALK indices w in [0, batch); the memory row of w is w, or batch - 1 - w when the launch is mirrored.  A launch on
// the buffer its predecessor wrote walks the other way: the rows written last are read first, while they may still be close to the chip.
// Rows with w >= keep_from are stored with the default cache policy instead of the streaming one.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kofft {
namespace host {

// What a context remembers of its last kClaim launch: the byte range it WROTE and the direction it walked.  bytes == 0: no record.
// Other launches through the context leave it alone: a stale record costs at most one needless flip, never a wrong result (rows are
// independent), and a caller that alternates this transform with pointwise kernels of its own on one buffer -- the case the rule is for --
// is indistinguishable from one whose other kernels came through the context.
struct PersistWalkRecord {
    uintptr_t lo = 0;
    size_t bytes = 0;
    bool mirrored = false;
};

enum : int { kPersistWalkRule = -1, kPersistWalkParent = 0, kPersistWalkAscKeep = 1, kPersistWalkDescKeep = 2 };
// (round 9: profiles/r09_walk_copy_model.txt and the T sweep in the kernel)
constexpr size_t kPersistKeepDefaultBytes = size_t(256) << 20;

inline bool persist_walk_is(const PersistWalkRecord &r, uintptr_t p, size_t bytes) { return r.bytes != 0 && r.lo == p && r.bytes == bytes; }

// The rule (mode -1): mirrored relative to the record when the input range or the output range is EXACTLY the recorded range, ascending
// otherwise -- a call on a fresh buffer, an overlapping but different range, a changed size and a cleared record are all "ascending".
inline bool persist_walk_rule(const PersistWalkRecord &r, uintptr_t in, size_t in_bytes, uintptr_t out, size_t out_bytes)
{
    return (persist_walk_is(r, in, in_bytes) || persist_walk_is(r, out, out_bytes)) ? !r.mirrored : false;
}

// First walk index of the kept zone; `batch` = no kept zone.  Under the rule the zone is switched off when the batch is smaller than
// twice the zone (what is kept then pushes out what the next call reads first no later than it helps); the forced modes (tests, A/B)
// clamp it to the batch instead, so that every position of keep_from can be reached at small batches.
inline size_t persist_keep_from(size_t batch, size_t row_bytes, size_t keep_bytes, bool clamp)
{
    if (row_bytes == 0 || batch == 0) return batch;
    const size_t rows = keep_bytes / row_bytes;
    if (rows == 0) return batch;
    if (clamp) return rows >= batch ? 0 : batch - rows;
    return rows > batch / 2 ? batch : batch - rows;
}

inline size_t persist_mem_row(size_t batch, size_t w, bool mirror) { return mirror ? batch - 1 - w : w; }

struct PersistWalkPlan {
    bool mirror;
    size_t keep_from;
};

inline PersistWalkPlan persist_walk_plan(int mode, const PersistWalkRecord &r, uintptr_t in, size_t in_bytes, uintptr_t out, size_t out_bytes,
                                         size_t batch, size_t row_bytes, size_t keep_bytes)
{
    switch (mode) {
    case kPersistWalkParent: return {false, batch};
    case kPersistWalkAscKeep: return {false, persist_keep_from(batch, row_bytes, keep_bytes, true)};
    case kPersistWalkDescKeep: return {true, persist_keep_from(batch, row_bytes, keep_bytes, true)};
    default: return {persist_walk_rule(r, in, in_bytes, out, out_bytes), persist_keep_from(batch, row_bytes, keep_bytes, false)};
    }
}

}  // namespace host
}  // namespace kofft
