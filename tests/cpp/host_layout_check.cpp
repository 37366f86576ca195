// host_layout_check.cpp -- properties of the host staging layout (kofft_amd/csrc/host_layout.h) over seeded random array sets,
// built with -fsanitize=address,undefined by tests/test_host_layout.py.  The pieces are laid into a real buffer of `total` bytes and
// every chunk of every array is written through, so an offset or a chunk that leaves its piece is also a sanitizer report.
// Then the scratch-chunk helper of the device routes' chunk loops (scratch_chunk_rows), the parser of its size knob and the dispatch
// over a log2 (dispatch_log2).
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
    // ---- scratch_chunk_rows: rows per piece of a chunk loop under a scratch cap.  The pieces are written into a scratch of exactly
    // `cap` bytes (one row where a row alone is larger) and counted off against the rows: a piece past the cap is a sanitizer report.
    const size_t caps[] = {1, 255, 4096, size_t(1) << 20, (size_t(1) << 20) + 1, size_t(8) << 20, kScratchChunkDefaultBytes, 2 * kScratchChunkDefaultBytes};
    for (int it = 0; it < 6000; ++it) {
        const size_t cap = (it % 3 == 0) ? draw(1, 70000) : caps[rng() % (sizeof(caps) / sizeof(caps[0]))];
        const size_t row_bytes = (it % 11 == 0) ? 0 : (it % 5 == 0) ? draw(cap / 2 + 1, 2 * cap + 8) : draw(1, cap < 64 ? 64 : cap < 40000 ? cap : 40000);
        const size_t count = (it % 13 == 0) ? 0 : (it % 4 == 0) ? draw(1, 4) : draw(1, 3000);
        const size_t chunk = scratch_chunk_rows(cap, row_bytes, count);
        if (count == 0) {
            CHECK(chunk == 0, "chunk case %d: %zu rows per piece of an empty batch", it, chunk);
            continue;
        }
        CHECK(chunk >= 1 && chunk <= count, "chunk case %d: %zu rows per piece of %zu rows", it, chunk, count);
        if (row_bytes == 0) {  // nothing to hold: one piece
            CHECK(chunk == count, "chunk case %d: rows of no bytes in pieces of %zu, not %zu", it, chunk, count);
            continue;
        }
        if (row_bytes > cap) CHECK(chunk == 1, "chunk case %d: a row of %zu bytes over the cap %zu in pieces of %zu", it, row_bytes, cap, chunk);
        else CHECK(chunk * row_bytes <= cap, "chunk case %d: %zu rows of %zu bytes exceed the cap %zu", it, chunk, row_bytes, cap);
        // (the largest that fits: one more row would pass the cap or the batch)
        CHECK(chunk == count || (chunk + 1) * row_bytes > cap, "chunk case %d: %zu rows per piece where %zu fit", it, chunk, chunk + 1);
        if (problems || chunk == 0) continue;
        // the loop of every route: for (b0 = 0; b0 < count; b0 += chunk) nb = min(chunk, count - b0)
        const bool small = cap <= 70000 && row_bytes <= cap;
        std::vector<unsigned char> scratch(small ? cap : 1, 0);
        size_t next = 0, pieces = 0;
        for (size_t b0 = 0; b0 < count; b0 += chunk, ++pieces) {
            const size_t nb = count - b0 < chunk ? count - b0 : chunk;
            CHECK(b0 == next && nb >= 1, "chunk case %d: piece %zu starts at row %zu after %zu", it, pieces, b0, next);
            next = b0 + nb;
            if (small) std::memset(scratch.data(), (int)(pieces + 1), nb * row_bytes);  // rows b0 .. at the head of the scratch
        }
        CHECK(next == count, "chunk case %d: the pieces end at row %zu of %zu", it, next, count);
        CHECK(pieces == (count + chunk - 1) / chunk, "chunk case %d: %zu pieces", it, pieces);
    }
    // the values the dispatch comments and the GPU seam tests count on
    CHECK(scratch_chunk_rows(kScratchChunkDefaultBytes, 8, 7) == 7 && scratch_chunk_rows(size_t(1) << 20, 4000, 1000) == 262 &&
              scratch_chunk_rows(size_t(1) << 20, 8000, 1000) == 131 && scratch_chunk_rows(size_t(1) << 20, size_t(1) << 21, 3) == 1,
          "scratch_chunk_rows: known values");

    // ---- KOFFT_HIP_SCRATCH_CHUNK_MB: 1 .. 512 MiB set the size, anything else leaves it alone
    {
        const size_t untouched = 12345;
        struct { const char *text; bool ok; size_t mb; } cases[] = {
            {"1", true, 1}, {"512", true, 512}, {"8", true, 8}, {"160", true, 160}, {"007", true, 7},
            {"0", false, 0}, {"-3", false, 0}, {"513", false, 0}, {"junk", false, 0}, {"", false, 0}, {"12x", false, 0}, {" 4", false, 0},
            {"4 ", false, 0}, {"+4", false, 0}, {"1.5", false, 0}, {"99999999999999999999999999", false, 0}, {"0x10", false, 0}};
        for (const auto &c : cases) {
            size_t bytes = untouched;
            const bool ok = parse_scratch_chunk_mb(c.text, &bytes);
            CHECK(ok == c.ok, "knob \"%s\": %s", c.text, ok ? "accepted" : "refused");
            CHECK(bytes == (c.ok ? c.mb << 20 : untouched), "knob \"%s\": %zu bytes", c.text, bytes);
        }
        size_t bytes = untouched;
        CHECK(!parse_scratch_chunk_mb(nullptr, &bytes) && bytes == untouched, "knob: a null string");
        CHECK(kScratchChunkDefaultBytes == (size_t)kScratchChunkMaxMb << 20, "the default is the ceiling");
    }
    // ---- dispatch_log2: every l of [LO, HI] reaches the instance of its own L and no other, an l outside reaches none and gives the
    // default (KOFFT_ERR_UNSUPPORTED or the caller's); a range of one value.  (the calls stand in parentheses of their own: the comma of
    // the template arguments would split CHECK's)
    {
        int calls = 0;
        auto own = [&](auto l) { return ++calls, 1000 + decltype(l)::value; };
        for (int l = 5; l <= 12; ++l) CHECK((dispatch_log2<5, 12>(l, own)) == 1000 + l, "dispatch_log2<5, 12>(%d)", l);
        CHECK(calls == 8, "dispatch_log2<5, 12>: %d calls for 8 lengths", calls);
        for (int l : {4, 13, 0, -1, 1 << 20}) {
            CHECK((dispatch_log2<5, 12>(l, own)) == KOFFT_ERR_UNSUPPORTED, "dispatch_log2<5, 12>(%d): not the default", l);
            CHECK((dispatch_log2<5, 12>(l, own, 77)) == 77, "dispatch_log2<5, 12>(%d): not the caller's default", l);
        }
        CHECK(calls == 8, "dispatch_log2<5, 12>: a call for a length outside the range");
        CHECK((dispatch_log2<7, 7>(7, own)) == 1007 && calls == 9, "dispatch_log2<7, 7>(7)");
        CHECK((dispatch_log2<7, 7>(6, own)) == KOFFT_ERR_UNSUPPORTED && (dispatch_log2<7, 7>(8, own, 0)) == 0 && calls == 9, "dispatch_log2<7, 7>: outside");
        // (a body that names an instance outside [LO, HI] does not compile: the static_assert is the "nothing else" check)
        auto only = [](auto l) {
            static_assert(decltype(l)::value >= 6 && decltype(l)::value <= 11, "an instance outside the range");
            return (int)decltype(l)::value;
        };
        for (int l = 6; l <= 11; ++l) CHECK((dispatch_log2<6, 11>(l, only)) == l, "dispatch_log2<6, 11>(%d)", l);
    }
    std::printf("%d problems\n", problems);
    return problems ? 1 : 0;
}
