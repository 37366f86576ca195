// host_layout_check.cpp -- properties of the host staging layout (kofft_amd/csrc/host_layout.h) over seeded random array sets,
// built with -fsanitize=address,undefined by tests/test_host_layout.py.  The pieces are laid into a real buffer of `total` bytes and
// every chunk of every array is written through, so an offset or a chunk that leaves its piece is also a sanitizer report.
#include "../../kofft_amd/csrc/host_layout.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace kofft::host;

static int problems = 0;
#define CHECK(cond, ...) \
    do { if (!(cond) && ++problems <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    std::mt19937_64 rng(20260517);
    auto draw = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };
    for (int it = 0; it < 3000; ++it) {
        const int n = (int)draw(1, kMaxHostArrays);
        const size_t elem = (it & 1) ? 8 : 4;
        const size_t batch = (it % 7 == 0) ? 0 : draw(0, 300);
        const size_t side_bytes = (it % 3 == 0) ? 0 : draw(1, 5000) * elem;
        size_t row[kMaxHostArrays];
        for (int k = 0; k < n; ++k) row[k] = (rng() % 5 == 0) ? 0 : draw(0, 5000);
        const HostLayout l = host_layout(n, row, batch, elem, side_bytes);
        CHECK(l.total >= 1, "set %d: total 0", it);
        std::vector<unsigned char> buf(l.total, 0);
        // pieces: the arrays, then the side input
        size_t off[kMaxHostArrays + 1], len[kMaxHostArrays + 1];
        for (int k = 0; k < n; ++k) {
            off[k] = l.off[k];
            len[k] = batch * row[k] * elem;
        }
        off[n] = l.side;
        len[n] = side_bytes;
        for (int k = 0; k <= n; ++k) {
            CHECK(off[k] % 256 == 0, "set %d piece %d: offset %zu not 256-byte aligned", it, k, off[k]);
            CHECK(off[k] < l.total, "set %d piece %d: offset %zu not below the total %zu", it, k, off[k], l.total);
            CHECK(off[k] + len[k] <= l.total, "set %d piece %d: ends at %zu, past the total %zu", it, k, off[k] + len[k], l.total);
            for (int j = 0; j < k; ++j)
                CHECK(off[j] + len[j] <= off[k] || off[k] + len[k] <= off[j] || !len[j] || !len[k], "set %d: pieces %d and %d overlap", it, j, k);
        }
        if (problems) continue;  // (the writes below trust the offsets)
        // the chunks of every array tile its piece exactly: each starts where the one before ended, the first at the piece's offset,
        // the last ends with the piece
        for (int parts : {0, 1, 3, 8, 64}) {
            const size_t chunk = host_chunk_rows(batch, parts);
            const size_t nchunks = chunk ? (batch + chunk - 1) / chunk : 0;
            CHECK(batch == 0 || (chunk >= 1 && nchunks <= (size_t)(parts > 0 ? parts : 8)), "set %d: %zu chunks for %d parts", it, nchunks, parts);
            for (int k = 0; k < n; ++k) {
                size_t next = off[k];
                for (size_t c = 0; c < nchunks; ++c) {
                    const size_t rows = batch - c * chunk < chunk ? batch - c * chunk : chunk;
                    const size_t at = off[k] + c * chunk * row[k] * elem, nb = rows * row[k] * elem;
                    CHECK(at == next && at + nb <= off[k] + len[k], "set %d array %d chunk %zu of %d parts: [%zu, %zu) does not follow %zu inside its piece",
                          it, k, c, parts, at, at + nb, next);
                    next = at + nb;
                    if (parts == 0 && at + nb <= buf.size()) std::memset(buf.data() + at, k + 1, nb);
                }
                CHECK(next == off[k] + len[k], "set %d array %d, %d parts: the chunks end at %zu, the piece at %zu", it, k, parts, next, off[k] + len[k]);
            }
        }
        // ... and wrote nothing but their own piece
        for (int k = 0; k <= n; ++k)
            for (size_t b = 0; b < len[k]; b += 97)
                CHECK(buf[off[k] + b] == (k < n ? k + 1 : 0), "set %d piece %d: byte %zu holds %d", it, k, b, (int)buf[off[k] + b]);
    }
    std::printf("%d problems\n", problems);
    return problems ? 1 : 0;
}
