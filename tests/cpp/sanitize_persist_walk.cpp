// sanitize_persist_walk.cpp -- kofft_amd/csrc/persist_walk.h in a stand-alone program that tests/test_persist_walk_cpu.py builds with
// -fsanitize=address,undefined.
//  * the direction rule's table: fresh context, same input range, same output range, overlapping but not equal, size changed, record
//    cleared, and the alternation of a chain of calls on one buffer;
//  * the four modes of persist_walk_plan;
//  * keep_from and the mirrored row at batches 1, 1024, 2^31 and 2^40, with zones of 0 bytes, one row, half the batch and more than it;
//  * for a few thousand seeded (batch, split) pairs: w -> persist_mem_row is a permutation of [0, batch), maps the walked part
//    [0, split) and the claimed part [split, batch) onto disjoint ranges, and is its own inverse.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../kofft_amd/csrc/persist_walk.h"

using namespace kofft::host;

static long problems = 0;
#define EXPECT(c)                                                 \
    do {                                                          \
        if (!(c)) {                                               \
            ++problems;                                           \
            std::printf("line %d: %s\n", __LINE__, #c);           \
        }                                                         \
    } while (0)

int main()
{
    const uintptr_t A = 0x7f0000000000ull, B = 0x7f0100000000ull;
    const size_t S = size_t(2) << 30;
    // ---- the rule
    {
        PersistWalkRecord none;
        EXPECT(!persist_walk_rule(none, A, S, A, S));                      // fresh
        EXPECT(!persist_walk_rule(none, 0, 0, 0, 0));                      // (an empty call never matches "no record")
        PersistWalkRecord asc{A, S, false}, desc{A, S, true};
        EXPECT(persist_walk_rule(asc, A, S, A, S));                        // in place on what was written
        EXPECT(!persist_walk_rule(desc, A, S, A, S));                      // ... and back
        EXPECT(persist_walk_rule(asc, A, S, B, S));                        // same input (ping-pong)
        EXPECT(persist_walk_rule(asc, B, S, A, S));                        // same output (the twin: same destination again)
        EXPECT(!persist_walk_rule(desc, B, S, A, S));
        EXPECT(!persist_walk_rule(asc, B, S, B, S));                       // another buffer
        EXPECT(!persist_walk_rule(asc, A + 4096, S, A + 4096, S));         // overlapping, not equal
        EXPECT(!persist_walk_rule(desc, A + 4096, S - 4096, B, S - 4096));
        EXPECT(!persist_walk_rule(asc, A, S / 2, A, S / 2));               // size changed
        EXPECT(!persist_walk_rule(asc, A, S + 32768, A, S + 32768));
        PersistWalkRecord cleared{A, 0, true};
        EXPECT(!persist_walk_rule(cleared, A, S, A, S));                   // record cleared
        EXPECT(!persist_walk_rule(cleared, A, 0, A, 0));
        // a chain on one buffer alternates; another buffer in between starts over
        PersistWalkRecord r;
        bool want = false;
        for (int k = 0; k < 9; ++k) {
            const PersistWalkPlan p = persist_walk_plan(kPersistWalkRule, r, A, S, A, S, 65536, 32768, 0);
            EXPECT(p.mirror == want && p.keep_from == 65536);
            r = PersistWalkRecord{A, S, p.mirror};
            want = !want;
        }
        const PersistWalkPlan other = persist_walk_plan(kPersistWalkRule, r, B, S, B, S, 65536, 32768, 0);
        EXPECT(!other.mirror);
    }
    // ---- the modes
    {
        const PersistWalkRecord asc{A, S, false};
        const size_t keep = size_t(64) << 20;
        PersistWalkPlan p = persist_walk_plan(kPersistWalkParent, asc, A, S, A, S, 65536, 32768, keep);
        EXPECT(!p.mirror && p.keep_from == 65536);
        p = persist_walk_plan(kPersistWalkAscKeep, asc, A, S, A, S, 65536, 32768, keep);
        EXPECT(!p.mirror && p.keep_from == 65536 - 2048);
        p = persist_walk_plan(kPersistWalkDescKeep, PersistWalkRecord{}, A, S, A, S, 65536, 32768, keep);
        EXPECT(p.mirror && p.keep_from == 65536 - 2048);
        p = persist_walk_plan(kPersistWalkRule, asc, A, S, A, S, 65536, 32768, keep);
        EXPECT(p.mirror && p.keep_from == 65536 - 2048);
        // twice the zone: 4096 rows keep 2048, 4095 rows keep none under the rule and 2048 when forced
        p = persist_walk_plan(kPersistWalkRule, asc, B, S, B, S, 4096, 32768, keep);
        EXPECT(!p.mirror && p.keep_from == 2048);
        p = persist_walk_plan(kPersistWalkRule, asc, B, S, B, S, 4095, 32768, keep);
        EXPECT(p.keep_from == 4095);
        p = persist_walk_plan(kPersistWalkAscKeep, asc, B, S, B, S, 4095, 32768, keep);
        EXPECT(p.keep_from == 2047);
    }
    // ---- keep_from and the mirror at the ends of the range
    const size_t batches[] = {1, 1024, size_t(1) << 31, size_t(1) << 40};
    for (const size_t batch : batches) {
        const size_t row = 32768;
        for (const bool clamp : {false, true}) {
            EXPECT(persist_keep_from(batch, row, 0, clamp) == batch);
            EXPECT(persist_keep_from(batch, row, row - 1, clamp) == batch);  // less than a row: none
            EXPECT(persist_keep_from(batch, 0, row, clamp) == batch);
            EXPECT(persist_keep_from(0, row, row, clamp) == 0);
            const size_t k1 = persist_keep_from(batch, row, row, clamp);  // one row
            EXPECT(k1 == (batch >= 2 || clamp ? batch - 1 : batch));
            const size_t half = persist_keep_from(batch, row, batch / 2 * row, clamp);
            EXPECT(half == (batch / 2 ? batch - batch / 2 : batch));
            const size_t over = persist_keep_from(batch, row, batch / 2 * row + row, clamp);  // one row more than half
            EXPECT(over == (clamp ? (batch / 2 + 1 >= batch ? 0 : batch - batch / 2 - 1) : batch));
            const size_t huge = persist_keep_from(batch, row, ~size_t(0), clamp);  // more than the batch
            EXPECT(huge == (clamp ? 0 : batch));
            EXPECT(k1 <= batch && half <= batch && over <= batch && huge <= batch);
        }
        EXPECT(persist_mem_row(batch, 0, false) == 0 && persist_mem_row(batch, batch - 1, false) == batch - 1);
        EXPECT(persist_mem_row(batch, 0, true) == batch - 1 && persist_mem_row(batch, batch - 1, true) == 0);
        EXPECT(persist_mem_row(batch, batch / 2, true) == batch - 1 - batch / 2);
    }
    // ---- the mirrored row is a permutation
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    long pairs = 0;
    for (int it = 0; it < 4000; ++it) {
        const size_t batch = 1 + next() % 3000;
        const size_t stride = 1 + next() % 600;
        const size_t split = next() % (batch + 1) / stride * stride;
        std::vector<int> seen(batch, 0);
        size_t lo_walked = batch, hi_walked = 0, lo_claimed = batch, hi_claimed = 0;
        for (size_t w = 0; w < batch; ++w) {
            const size_t m = persist_mem_row(batch, w, true);
            if (m >= batch) {
                ++problems;
                continue;
            }
            ++seen[m];
            if (persist_mem_row(batch, m, true) != w || persist_mem_row(batch, w, false) != w) ++problems;
            size_t &lo = w < split ? lo_walked : lo_claimed, &hi = w < split ? hi_walked : hi_claimed;
            lo = m < lo ? m : lo;
            hi = m > hi ? m : hi;
        }
        for (size_t m = 0; m < batch; ++m)
            if (seen[m] != 1) ++problems;
        if (split > 0 && split < batch && !(hi_claimed < lo_walked)) ++problems;  // mirrored: the claimed part lies below the walked part
        ++pairs;
    }
    std::printf("persist_walk: %ld (batch, split) pairs, %ld problems\n", pairs, problems);
    return problems ? 1 : 0;
}
