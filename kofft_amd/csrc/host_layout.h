// host_layout.h -- where the arrays of one host-pointer call lie in its staging buffer (kofft_hip.hip: stage_host).
// Arithmetic only, no HIP: tests/cpp/host_layout_check.cpp includes this file alone.
#pragma once
#include <cstddef>

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

}  // namespace host
}  // namespace kofft
