// host_cache_check.cpp -- the table cache, the grow-only scratch and the resident-grid size of kofft_amd/csrc/host_cache.h on a malloc /
// free allocator that fails the k-th allocation on request, built with -fsanitize=address,undefined by tests/test_host_cache.py.
// The tables and buffers are real heap blocks, written through: a pointer that outlives its block, a block freed twice or one that
// nothing frees (LeakSanitizer, at exit) is a sanitizer report.
#include "../../kofft_amd/csrc/host_cache.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using namespace kofft::host;

static int problems = 0;
#define CHECK(cond, ...) \
    do { if (!(cond) && ++problems <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct TestAlloc {
    static int allocs, frees, fail_at;  // fail_at: the allocation (counted from 1 after arm()) that fails; 0: none
    static void arm(int k) { allocs = frees = 0; fail_at = k; }
    static const char *alloc(void **p, size_t bytes)
    {
        if (++allocs == fail_at) return "injected failure";
        *p = std::malloc(bytes ? bytes : 1);
        return *p ? nullptr : "malloc";
    }
    static const char *free(void *p)
    {
        ++frees;
        std::free(p);
        return nullptr;
    }
};
int TestAlloc::allocs = 0, TestAlloc::frees = 0, TestAlloc::fail_at = 0;

struct Ctx {
    TableCache tables;
    std::string last_error;
    ~Ctx() { for (auto &kv : tables) std::free(kv.second); }  // as kofft_hip_destroy: every cached table once
};

static int builds = 0;
// fills the table, like an upload
static auto fill(size_t bytes, int value) { return [=](void *d, std::string &) { ++builds; std::memset(d, value, bytes); return KOFFT_OK; }; }
static auto fill2(size_t ba, size_t bb) { return [=](void *a, void *b, std::string &) { ++builds; std::memset(a, 1, ba); std::memset(b, 2, bb); return KOFFT_OK; }; }

int main()
{
    // ---- one table: build, hit, the three ways to fail, retry ---------------------------------------------------------------------------
    {
        Ctx ctx;
        void *p = nullptr, *q = nullptr;
        TestAlloc::arm(0);
        builds = 0;
        CHECK(cached_table<TestAlloc>(&ctx, kTableTwF32, 64, 256, "t", &p, fill(256, 7)) == KOFFT_OK && p && builds == 1, "first call builds");
        CHECK(cached_table<TestAlloc>(&ctx, kTableTwF32, 64, 256, "t", &q, fill(256, 9)) == KOFFT_OK && q == p && builds == 1, "a hit returns the first pointer, no build");
        CHECK(TestAlloc::allocs == 1 && TestAlloc::frees == 0 && static_cast<unsigned char *>(q)[255] == 7, "a hit allocates nothing");
        CHECK(cached_table<TestAlloc>(&ctx, kTableTwF32, 128, 512, "t", &q, fill(512, 1)) == KOFFT_OK && q != p && builds == 2, "another n is another table");
        CHECK(cached_table<TestAlloc>(&ctx, kTableTwF64, 64, 512, "t", &q, fill(512, 1)) == KOFFT_OK && q != p && builds == 3, "another kind is another table");
        const TableCache before = ctx.tables;
        // the builder fails
        TestAlloc::arm(0);
        q = &ctx;
        int rc = cached_table<TestAlloc>(&ctx, kTableHann, 100, 400, "window upload", &q, [](void *d, std::string &why) {
            std::memset(d, 3, 400);
            why = "no route to device";
            return KOFFT_ERR_HIP;
        });
        CHECK(rc == KOFFT_ERR_HIP && q == nullptr && ctx.tables == before && TestAlloc::allocs == 1 && TestAlloc::frees == 1, "builder failure: freed, not cached");
        CHECK(ctx.last_error == "window upload: no route to device", "builder failure text: %s", ctx.last_error.c_str());
        // the builder runs out of host memory
        TestAlloc::arm(0);
        rc = cached_table<TestAlloc>(&ctx, kTableHann, 100, 400, "window upload", &q, [](void *, std::string &) -> int { throw std::bad_alloc(); });
        CHECK(rc == KOFFT_ERR_ALLOC && q == nullptr && ctx.tables == before && TestAlloc::frees == 1, "bad_alloc in the builder: freed, not cached");
        // the allocation fails: the builder never runs
        TestAlloc::arm(1);
        builds = 0;
        rc = cached_table<TestAlloc>(&ctx, kTableHann, 100, 400, "window upload", &q, fill(400, 3));
        CHECK(rc == KOFFT_ERR_HIP && q == nullptr && ctx.tables == before && builds == 0 && TestAlloc::frees == 0, "allocation failure: nothing built or cached");
        CHECK(ctx.last_error == "window upload: allocation: injected failure", "allocation failure text: %s", ctx.last_error.c_str());
        // the retry succeeds and is cached
        TestAlloc::arm(0);
        CHECK(cached_table<TestAlloc>(&ctx, kTableHann, 100, 400, "window upload", &p, fill(400, 3)) == KOFFT_OK && p && builds == 1, "retry builds");
        CHECK(cached_table<TestAlloc>(&ctx, kTableHann, 100, 400, "window upload", &q, fill(400, 3)) == KOFFT_OK && q == p && builds == 1, "retry is cached");
        CHECK(ctx.tables.size() == before.size() + 1, "one more table");
        // a builder may use the cache for other keys (Bluestein's fft(b) fetches the twiddles of m)
        rc = cached_table<TestAlloc>(&ctx, kTableDct2, 5, 40, "outer", &p, [&](void *d, std::string &) {
            void *inner = nullptr;
            std::memset(d, 5, 40);
            return cached_table<TestAlloc>(&ctx, kTableTwF32, 8, 32, "inner", &inner, fill(32, 6));
        });
        CHECK(rc == KOFFT_OK && ctx.tables.count({kTableDct2, 5}) && ctx.tables.count({kTableTwF32, 8}), "nested build");
    }
    // ---- a pair: both or neither ---------------------------------------------------------------------------------------------------------
    {
        Ctx ctx;
        void *a = nullptr, *b = nullptr, *a2 = nullptr, *b2 = nullptr;
        for (int fail = 1; fail <= 2; ++fail) {  // the first, then the second allocation of the pair fails
            TestAlloc::arm(fail);
            builds = 0;
            const int rc = cached_table_pair<TestAlloc>(&ctx, kTableBlueChirpF32, kTableBlueBfftF32, 100, 800, 2048, "pair", &a, &b, fill2(800, 2048));
            CHECK(rc == KOFFT_ERR_HIP && !a && !b && ctx.tables.empty() && builds == 0 && TestAlloc::frees == fail - 1, "pair: allocation %d fails", fail);
        }
        TestAlloc::arm(0);
        int rc = cached_table_pair<TestAlloc>(&ctx, kTableBlueChirpF32, kTableBlueBfftF32, 100, 800, 2048, "bluestein tables", &a, &b,
                                              [](void *da, void *db, std::string &why) {
                                                  std::memset(da, 1, 800);  // the first table is up, the second one's step fails
                                                  std::memset(db, 2, 2048);
                                                  why = "fft(b): failed";
                                                  return KOFFT_ERR_HIP;
                                              });
        CHECK(rc == KOFFT_ERR_HIP && !a && !b && ctx.tables.empty() && TestAlloc::frees == 2, "pair: second half fails, both freed");
        CHECK(ctx.last_error == "bluestein tables: fft(b): failed", "pair failure text: %s", ctx.last_error.c_str());
        rc = cached_table_pair<TestAlloc>(&ctx, kTableBlueChirpF32, kTableBlueBfftF32, 100, 800, 2048, "pair", &a, &b,
                                          [](void *, void *, std::string &) -> int { throw std::bad_alloc(); });
        CHECK(rc == KOFFT_ERR_ALLOC && ctx.tables.empty(), "pair: bad_alloc in the builder");
        builds = 0;
        rc = cached_table_pair<TestAlloc>(&ctx, kTableBlueChirpF32, kTableBlueBfftF32, 100, 800, 2048, "pair", &a, &b, fill2(800, 2048));
        CHECK(rc == KOFFT_OK && a && b && a != b && ctx.tables.size() == 2 && builds == 1, "pair: retry builds both");
        const int allocs_before = TestAlloc::allocs;
        rc = cached_table_pair<TestAlloc>(&ctx, kTableBlueChirpF32, kTableBlueBfftF32, 100, 800, 2048, "pair", &a2, &b2, fill2(800, 2048));
        CHECK(rc == KOFFT_OK && a2 == a && b2 == b && builds == 1 && TestAlloc::allocs == allocs_before, "pair: hit");
        CHECK(static_cast<unsigned char *>(a)[799] == 1 && static_cast<unsigned char *>(b)[2047] == 2, "pair: contents");
    }
    // ---- kinds: all distinct, the direct enumerators are their arithmetic, f64 follows f32 ------------------------------------------------
    {
        const TableKind all[] = {kTableTwF32, kTableTwF64, kTableRfftF32, kTableRfftF64, kTableHann, kTableBlueChirpF32, kTableBlueChirpF64,
                                 kTableBlueBfftF32, kTableBlueBfftF64, kTableRadix4PermF32, kTableRadix4PermF64, kTableRadix4TwF32,
                                 kTableRadix4TwF64, kTableDct2, kTableDct1Direct, kTableDct2Direct, kTableDct3Direct, kTableDct4Direct,
                                 kTableDst1Direct, kTableDst2Direct, kTableDst3Direct, kTableDst4Direct, kTableDht};
        std::set<int> seen;
        for (TableKind k : all) CHECK(seen.insert(int(k)).second, "kind %d twice", int(k));
        const TableKind direct[2][4] = {{kTableDct1Direct, kTableDct2Direct, kTableDct3Direct, kTableDct4Direct},
                                        {kTableDst1Direct, kTableDst2Direct, kTableDst3Direct, kTableDst4Direct}};
        std::set<int> rest = seen;
        for (int f = 0; f < 2; ++f)
            for (int t = 1; t <= 4; ++t) {
                CHECK(direct_table_kind(f, t) == direct[f][t - 1], "direct kind (%d, %d)", f, t);
                CHECK(rest.erase(int(direct_table_kind(f, t))) == 1, "direct kind (%d, %d) not among the kinds", f, t);
            }
        CHECK(rest.size() == seen.size() - 8, "eight direct kinds, none of them another table's");
        CHECK(kind_for<float>(kTableTwF32) == kTableTwF32 && kind_for<double>(kTableTwF32) == kTableTwF64 &&
                  kind_for<double>(kTableRfftF32) == kTableRfftF64 && kind_for<double>(kTableBlueChirpF32) == kTableBlueChirpF64 &&
                  kind_for<double>(kTableBlueBfftF32) == kTableBlueBfftF64 && kind_for<double>(kTableRadix4PermF32) == kTableRadix4PermF64 &&
                  kind_for<double>(kTableRadix4TwF32) == kTableRadix4TwF64,
              "kind_for");
    }
    // ---- ensure_buf: grows, never shrinks, a failure leaves nothing; a release loop frees each buffer once --------------------------------
    {
        Ctx ctx;
        DevBuf buf;
        TestAlloc::arm(0);
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 100) == KOFFT_OK && buf.p && buf.bytes == 100 && TestAlloc::allocs == 1, "ensure: first");
        std::memset(buf.p, 1, 100);
        void *first = buf.p;
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 40) == KOFFT_OK && buf.p == first && buf.bytes == 100, "ensure: never shrinks");
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 100) == KOFFT_OK && buf.p == first && TestAlloc::allocs == 1 && TestAlloc::frees == 0, "ensure: fits");
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 5000) == KOFFT_OK && buf.bytes == 5000 && TestAlloc::allocs == 2 && TestAlloc::frees == 1, "ensure: grows, old freed");
        std::memset(buf.p, 2, 5000);
        TestAlloc::arm(1);
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 6000) == KOFFT_ERR_HIP && buf.p == nullptr && buf.bytes == 0 && TestAlloc::frees == 1, "ensure: a failed growth leaves {nullptr, 0}");
        CHECK(ctx.last_error == "scratch: allocation: injected failure", "ensure failure text: %s", ctx.last_error.c_str());
        TestAlloc::arm(0);
        CHECK(ensure_buf<TestAlloc>(&ctx, buf, 6000) == KOFFT_OK && buf.bytes == 6000 && TestAlloc::frees == 0, "ensure: retry after a failure");
        std::memset(buf.p, 3, 6000);
        DevBuf other, never;
        CHECK(ensure_buf<TestAlloc>(&ctx, other, 10) == KOFFT_OK, "ensure: a second buffer");
        TestAlloc::arm(0);
        DevBuf *const list[] = {&buf, &other, &never};
        for (int round = 0; round < 2; ++round)  // (the second round: nothing left to free)
            for (DevBuf *b : list) release_buf<TestAlloc>(*b);
        CHECK(TestAlloc::frees == 2 && !buf.p && !buf.bytes && !other.p && !other.bytes && !never.p, "release: each buffer once");
    }
    // ---- resident_blocks ------------------------------------------------------------------------------------------------------------------
    {
        const struct { int cus, per_cu, pct; size_t need, want; } rows[] = {
            {256, 2, 0, 1000000, 512}, {256, 2, 50, 1000000, 256}, {256, 2, 150, 1000000, 768}, {256, 2, 0, 3, 3}, {1, 1, 1, 5, 1}, {256, 0, 0, 7, 1},
            {256, 2, -5, 1000000, 512}, {256, 3, 0, kNoNeedCap, 768}, {304, 1, 0, 304, 304}, {304, 1, 0, 303, 303}};
        for (const auto &r : rows) {
            const size_t got = resident_blocks(r.cus, r.per_cu, r.pct, r.need);
            CHECK(got == r.want, "resident_blocks(%d, %d, %d, %zu) = %zu, not %zu", r.cus, r.per_cu, r.pct, r.need, got, r.want);
        }
        for (int cus : {1, 7, 256, 304})
            for (int per_cu : {0, 1, 2, 3, 8})
                for (int pct : {0, 1, 33, 100, 250})
                    for (size_t need : {size_t(1), size_t(2), size_t(255), size_t(100000)}) {
                        const size_t got = resident_blocks(cus, per_cu, pct, need);
                        CHECK(got >= 1 && got <= need, "resident_blocks(%d, %d, %d, %zu) = %zu", cus, per_cu, pct, need, got);
                    }
    }
    std::printf("%d problems\n", problems);
    return problems ? 1 : 0;
}
