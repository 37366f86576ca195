// host_cache.h -- the host plumbing every transform family shares: the cache of device tables, the grow-only device scratch and the
// size of a chip-resident grid.  Logic only, no HIP: the device allocator is a policy -- hipMalloc / hipFree in the library
// (host_common.hip.h: HipAlloc), malloc / free with failure injection in tests/cpp/host_cache_check.cpp, which includes this file alone.
//   struct Alloc { static const char *alloc(void **p, size_t bytes);   // nullptr and *p set, or the failure's text and *p untouched
//                  static const char *free(void *p); };                // nullptr, or the failure's text
// Ctx is anything with `TableCache tables` and `std::string last_error` (kofft_hip_ctx).
#pragma once
#include "../../include/kofft_hip.h"

#include <cstddef>
#include <map>
#include <new>
#include <string>
#include <utility>

namespace kofft {
namespace host {

// ---- the table cache: (kind, n) -> device table, built at the first call that needs it and kept until the context is destroyed ----
// Every kind there is.  The F64 kind of a pair is the F32 one + 1.
enum TableKind : int {
    kTableTwF32 = 0,         // FftPlanner twiddles: n / 2 complex
    kTableTwF64 = 1,
    kTableRfftF32 = 2,       // RfftPlanner post-pass table: n complex
    kTableRfftF64 = 3,
    kTableHann = 4,          // hann(n): stft_magnitudes' window
    kTableBlueChirpF32 = 5,  // Bluestein: chirp (n complex) ...
    kTableBlueChirpF64 = 6,
    kTableBlueBfftF32 = 7,   // ... and fft(b) (m complex), built and cached together
    kTableBlueBfftF64 = 8,
    kTableRadix4PermF32 = 9,  // fft_radix4: the swap loop's net permutation (n unsigned) ...
    kTableRadix4PermF64 = 10,
    kTableRadix4TwF32 = 11,  // ... and every stage's (w1, w2, w3) triples, built and cached together
    kTableRadix4TwF64 = 12,
    kTableDct2 = 13,         // DctPlanner (cos, sin): n pairs, f32 only
    kTableDct4Fast = 14,     // the fast DCT-IV's pre- and post-twiddles: n / 2 + n / 2 pairs, f32 only
    // the n x ldc tables of the direct sums: kTableDirect + 4 * family + (type - 1), family 0 = DCT, 1 = DST (direct_table_kind)
    kTableDirect = 20,
    kTableDct1Direct = kTableDirect + 4 * 0 + 0,
    kTableDct2Direct = kTableDirect + 4 * 0 + 1,
    kTableDct3Direct = kTableDirect + 4 * 0 + 2,
    kTableDct4Direct = kTableDirect + 4 * 0 + 3,
    kTableDst1Direct = kTableDirect + 4 * 1 + 0,
    kTableDst2Direct = kTableDirect + 4 * 1 + 1,
    kTableDst3Direct = kTableDirect + 4 * 1 + 2,
    kTableDst4Direct = kTableDirect + 4 * 1 + 3,
    kTableDht = kTableDirect + 4 * 2,  // the Hartley table, n x ldc
};
constexpr TableKind direct_table_kind(int family, int type) { return TableKind(kTableDirect + 4 * family + (type - 1)); }
template <typename T>
constexpr TableKind kind_for(TableKind f32) { return sizeof(T) == 4 ? f32 : TableKind(f32 + 1); }

using TableCache = std::map<std::pair<int, size_t>, void *>;

// What every failure below leaves behind: "label: why" in ctx->last_error, rc to the caller.
template <class Ctx>
inline int report_failure(Ctx *ctx, int rc, const char *label, const std::string &why)
{
    ctx->last_error = std::string(label) + ": " + why;
    return rc;
}

// The table (kind, n) of `bytes` bytes.  A hit is one find.  A miss allocates, runs build(d, why) -> status on the fresh device pointer
// (an upload, a kernel on the context's stream, device work and a synchronisation; a failure's text goes into `why`) and caches the
// pointer only after build has returned KOFFT_OK; any failure frees the allocation, caches nothing and leaves "label: why" in
// ctx->last_error.  build may use the cache for other keys.
template <class Alloc, class P, class Ctx, class Build>
int cached_table(Ctx *ctx, TableKind kind, size_t n, size_t bytes, const char *label, P **out, Build build)
{
    const auto key = std::make_pair(int(kind), n);
    const auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        *out = static_cast<P *>(it->second);
        return KOFFT_OK;
    }
    *out = nullptr;
    void *d = nullptr;
    if (const char *bad = Alloc::alloc(&d, bytes)) return report_failure(ctx, KOFFT_ERR_HIP, label, std::string("allocation: ") + bad);
    std::string why;
    int rc;
    try {
        rc = build(d, why);
        if (rc == KOFFT_OK) ctx->tables[key] = d;
    } catch (const std::bad_alloc &) {
        rc = KOFFT_ERR_ALLOC;
        why = "out of host memory";
    }
    if (rc != KOFFT_OK) {
        (void)Alloc::free(d);
        return report_failure(ctx, rc, label, why);
    }
    *out = static_cast<P *>(d);
    return KOFFT_OK;
}

// Two tables that one builder makes, build(da, db, why): both cached or neither, so a hit is both finds and a miss builds both.
template <class Alloc, class P, class Q, class Ctx, class Build>
int cached_table_pair(Ctx *ctx, TableKind kind_a, TableKind kind_b, size_t n, size_t bytes_a, size_t bytes_b, const char *label, P **out_a,
                      Q **out_b, Build build)
{
    const auto key_a = std::make_pair(int(kind_a), n), key_b = std::make_pair(int(kind_b), n);
    const auto ia = ctx->tables.find(key_a), ib = ctx->tables.find(key_b);
    if (ia != ctx->tables.end() && ib != ctx->tables.end()) {
        *out_a = static_cast<P *>(ia->second);
        *out_b = static_cast<Q *>(ib->second);
        return KOFFT_OK;
    }
    *out_a = nullptr;
    *out_b = nullptr;
    void *da = nullptr, *db = nullptr;
    const char *bad = Alloc::alloc(&da, bytes_a);
    if (!bad) bad = Alloc::alloc(&db, bytes_b);
    std::string why = bad ? std::string("allocation: ") + bad : std::string();
    int rc = bad ? KOFFT_ERR_HIP : KOFFT_OK;
    if (!bad) {
        try {
            rc = build(da, db, why);
            if (rc == KOFFT_OK) {
                ctx->tables[key_a] = da;
                ctx->tables[key_b] = db;
            }
        } catch (const std::bad_alloc &) {
            ctx->tables.erase(key_a);  // (the second insertion threw)
            rc = KOFFT_ERR_ALLOC;
            why = "out of host memory";
        }
    }
    if (rc != KOFFT_OK) {
        if (da) (void)Alloc::free(da);
        if (db) (void)Alloc::free(db);
        return report_failure(ctx, rc, label, why);
    }
    *out_a = static_cast<P *>(da);
    *out_b = static_cast<Q *>(db);
    return KOFFT_OK;
}

// ---- grow-only device scratch ----------------------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// At least `bytes` in buf.  Growing frees the old buffer FIRST: with hipFree that is a device synchronisation, so nothing in flight still
// uses it (and the two never coexist).  A failed allocation leaves {nullptr, 0}.
template <class Alloc, class Ctx>
int ensure_buf(Ctx *ctx, DevBuf &buf, size_t bytes)
{
    if (buf.bytes >= bytes) return KOFFT_OK;
    if (buf.p) {
        if (const char *bad = Alloc::free(buf.p)) return report_failure(ctx, KOFFT_ERR_HIP, "scratch: free", bad);
    }
    buf = DevBuf{};
    void *p = nullptr;
    if (const char *bad = Alloc::alloc(&p, bytes)) return report_failure(ctx, KOFFT_ERR_HIP, "scratch: allocation", bad);
    buf.p = p;
    buf.bytes = bytes;
    return KOFFT_OK;
}

template <class Alloc>
void release_buf(DevBuf &buf)
{
    if (buf.p) (void)Alloc::free(buf.p);
    buf = DevBuf{};
}

// ---- workgroups of a chip-resident (persistent) grid: per_cu on each of num_cus CUs, scaled by the measurement knob grid_pct (percent;
// <= 0: off), at least one, no more than the `need` units of work there are (kNoNeedCap: the caller slices the grid itself) -------------
constexpr size_t kNoNeedCap = ~size_t(0);
inline size_t resident_blocks(int num_cus, int per_cu, int grid_pct, size_t need)
{
    size_t blocks = (size_t)num_cus * (size_t)per_cu;
    if (grid_pct > 0) blocks = blocks * (size_t)grid_pct / 100;
    if (blocks < 1) blocks = 1;
    return blocks > need ? need : blocks;
}

}  // namespace host
}  // namespace kofft
