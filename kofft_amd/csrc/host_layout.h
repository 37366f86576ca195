// host_layout.h -- where the arrays of one host-pointer call lie in its staging buffer (host_stage.hip.h: stage_host), the scratch chunks
// and their walk, the dispatch over a log2 and the overlap test of the device forms.  Arithmetic only, no HIP:
// tests/cpp/host_layout_check.cpp and tests/cpp/sanitize_frame_cut.cpp include this file alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/kofft_hip.h"  // (the status codes; plain C, no HIP)

namespace kofft {
namespace host {

constexpr int kMaxHostArrays = 4;

// Array k holds batch * row[k] elements at off[k], the side input follows at `side`; `total` bytes in all.  Every offset is a multiple
// of 256 and below `total`, also where a piece is empty: a device pointer made from it is never null and never past the buffer.
struct HostLayout {
    size_t off[kMaxHostArrays];
    size_t side;
    size_t total;
};

inline HostLayout host_layout(int n, const size_t *row, size_t batch, size_t elem, size_t side_bytes)
{
    HostLayout l{};
    size_t end = 0;
    for (int k = 0; k < n; ++k) {
        l.off[k] = (end + 255) & ~size_t(255);
        end = l.off[k] + batch * row[k] * elem;
    }
    l.side = (end + 255) & ~size_t(255);
    l.total = l.side + (side_bytes ? side_bytes : 1);
    return l;
}

// rows per chunk of a pipelined batch in `parts` pieces (0: the default, 8); chunk c of an array is its rows [c * chunk, ...)
inline size_t host_chunk_rows(size_t batch, int parts)
{
    const size_t p = (size_t)(parts > 0 ? parts : 8);
    return (batch + p - 1) / p;
}

// ---- scratch chunks: the host routes that work through a scratch buffer take a large batch in pieces of at most `cap_bytes` of it ----
// The default cap (kofft_hip_ctx::scratch_chunk_bytes) and the largest one KOFFT_HIP_SCRATCH_CHUNK_MB may set: the flat kernels' 32-bit
// index math (a chunk holds at most 2^27 floats) and the 0x7fffffff block checks of the chunk loops rest on this ceiling.
constexpr size_t kScratchChunkDefaultBytes = size_t(512) << 20;
constexpr long kScratchChunkMaxMb = 512;

// rows (transforms, blocks) per piece: cap_bytes / row_bytes, at least 1 (a row larger than the cap goes alone), at most `count`;
// count == 0: 0, no piece at all.  Piece k covers rows [k * chunk, min((k + 1) * chunk, count)).
inline size_t scratch_chunk_rows(size_t cap_bytes, size_t row_bytes, size_t count)
{
    if (count == 0) return 0;
    size_t chunk = row_bytes ? cap_bytes / row_bytes : count;
    if (chunk < 1) chunk = 1;
    return chunk > count ? count : chunk;
}

// The chunk walk: body(t0, nt) for the pieces [t0, t0 + nt) of [0, total), `chunk` at a time (chunk >= 1 where total > 0), in order;
// it ends at the first body that returns non-zero and returns that, otherwise 0.
template <class Body>
inline int for_chunks(size_t total, size_t chunk, Body &&body)
{
    for (size_t t0 = 0; t0 < total; t0 += chunk) {
        const int rc = body(t0, total - t0 < chunk ? total - t0 : chunk);
        if (rc) return rc;
    }
    return 0;
}

// ---- a run-time log2 to a compile-time one ----
// f(std::integral_constant<int, L>{}) for the L in [LO, HI] that equals l; `otherwise` (KOFFT_ERR_UNSUPPORTED) for an l outside.  f is
// a generic lambda that launches the kernel instance of 2^L points; exactly the instances LO .. HI exist.
template <int LO, int HI, class F>
inline int dispatch_log2(int l, F &&f, int otherwise = KOFFT_ERR_UNSUPPORTED)
{
    static_assert(LO <= HI, "an empty range");
    if (l == LO) return f(std::integral_constant<int, LO>{});
    if constexpr (LO < HI) return dispatch_log2<LO + 1, HI>(l, f, otherwise);
    else return otherwise;
}

// ---- the overlap checks of the device forms ----
// the bytes [a, a + a_bytes) and [b, b + b_bytes) share one; a null pointer or an empty range never does
inline bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p && q && a_bytes && b_bytes && p < q + b_bytes && q < p + a_bytes;
}

// elements from the first of row 0 to the last of row rows - 1 of a strided batch (row_stride >= len; it does not count when rows == 1)
inline size_t rows_span(size_t rows, size_t len, size_t row_stride) { return rows && len ? (rows - 1) * row_stride + len : 0; }

// KOFFT_HIP_SCRATCH_CHUNK_MB: a whole number of MiB from 1 to kScratchChunkMaxMb, nothing before or after it.  true: *bytes is set;
// false (empty, not a number, trailing text, out of range): *bytes is left alone.
inline bool parse_scratch_chunk_mb(const char *text, size_t *bytes)
{
    if (!text || !*text) return false;
    long mb = 0;
    for (const char *p = text; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        mb = mb * 10 + (*p - '0');
        if (mb > kScratchChunkMaxMb) return false;
    }
    if (mb < 1) return false;
    *bytes = (size_t)mb << 20;
    return true;
}

}  // namespace host
}  // namespace kofft
