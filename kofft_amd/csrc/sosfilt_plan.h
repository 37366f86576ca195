// sosfilt_plan.h -- the index arithmetic of the batched IIR filter.  A row of nx samples is walked sequentially,
// forwards or (KOFFT_HIP_SOSFILT_REVERSE) backwards; the tiled kernel cuts it into tiles of T samples on a grid that starts at sample
// 0 in both directions -- tile k holds samples [k * T, min(nx, (k + 1) * T)) -- and only the order of the tiles and of the samples
// inside a tile turns round.  A wavefront owns kSosRows consecutive rows; a cascade runs in passes of at most kSosGroup sections.
// Arithmetic only, no HIP header: the kernels (sosfilt_impl.hip.h) and the host (k_sosfilt_f32.hip) call these functions, and
// tests/cpp/sanitize_sosfilt_plan.cpp includes this file alone and compares them with an enumeration of every sample.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define KOFFT_SOS_HD __host__ __device__ inline
#else
#define KOFFT_SOS_HD inline
#endif

namespace kofft {
namespace host {

constexpr unsigned kSosRows = 64;   // rows of one wavefront of the tiled kernel: one per lane
#ifdef KOFFT_SOSFILT_MEASURE_TILE    // (a measurement build for tools/bench_sosfilt.py: another tile; the tests hold for the header's)
constexpr unsigned kSosTile = KOFFT_SOSFILT_MEASURE_TILE;
#else
constexpr unsigned kSosTile = 32;   // T: samples per tile (KOFFT_HIP_SOSFILT_TILE): 16, 32 or 64
#endif
#ifdef KOFFT_SOSFILT_MEASURE_PREFETCH  // (a measurement build: the next tile prefetched into registers, sosfilt_impl.hip.h)
constexpr bool kSosPrefetch = true;
#else
constexpr bool kSosPrefetch = false;
#endif
constexpr unsigned kSosGroup = 8;   // G: sections per pass (KOFFT_HIP_SOSFILT_GROUP)
constexpr unsigned kSosPlainThreads = 256;

// The measured rule behind kofft_hip_set_sosfilt_tiled(ctx, 1) (profiles/sosfilt_bench.txt): the tiled kernel from
// kSosTiledMinRows rows on -- it measured faster than the plain one, outside the spread of the rounds, at 16 rows and at every larger
// count tried, for 1 to 12 sections; at a single row it is faster with one section and inside the spread with eight.
constexpr unsigned long long kSosTiledMinRows = 16;
KOFFT_SOS_HD int sos_route(unsigned long long rows) { return rows >= kSosTiledMinRows ? 1 : 0; }

// tiles of a row of nx samples (nx >= 1)
KOFFT_SOS_HD unsigned long long sos_tiles(unsigned long long nx, unsigned tile) { return (nx - 1) / tile + 1; }

// the tile walked at step `step` of `ntiles`: ascending, or descending with the reverse flag
KOFFT_SOS_HD unsigned long long sos_tile_at(unsigned long long step, unsigned long long ntiles, bool reverse)
{
    return reverse ? ntiles - 1 - step : step;
}

// samples of tile `tile`: T, or what is left of the row in the last one.  Never 0 for tile < sos_tiles(nx, T).
KOFFT_SOS_HD unsigned sos_tile_len(unsigned long long tile, unsigned long long nx, unsigned T)
{
    const unsigned long long left = nx - tile * T;
    return left < T ? (unsigned)left : T;
}

// the sample inside a tile of `len` samples (or inside a whole row) walked at step i < len
KOFFT_SOS_HD unsigned long long sos_walk_at(unsigned long long i, unsigned long long len, bool reverse) { return reverse ? len - 1 - i : i; }

// groups of kSosRows rows of a batch (rows >= 1), and the rows of group `g`
KOFFT_SOS_HD unsigned long long sos_row_groups(unsigned long long rows) { return (rows - 1) / kSosRows + 1; }
KOFFT_SOS_HD unsigned sos_group_rows(unsigned long long g, unsigned long long rows)
{
    const unsigned long long left = rows - g * kSosRows;
    return left < kSosRows ? (unsigned)left : kSosRows;
}

// passes of a cascade of `sections` (>= 1) and the sections of pass `p`, which begins at section p * G
KOFFT_SOS_HD unsigned long long sos_passes(unsigned long long sections, unsigned G) { return (sections - 1) / G + 1; }
KOFFT_SOS_HD unsigned sos_pass_sections(unsigned long long p, unsigned long long sections, unsigned G)
{
    const unsigned long long left = sections - p * G;
    return left < G ? (unsigned)left : G;
}

// Element k of a tile of `len` samples of `nrows` rows, as the wavefront's coalesced copies count it (k = lane, lane + 64, ..): lanes run
// along time.  *r < kSosRows and *t < T always; the element exists where *r < nrows and *t < len.
KOFFT_SOS_HD void sos_tile_elem(unsigned k, unsigned T, unsigned *r, unsigned *t)
{
    *r = k / T;
    *t = k - *r * T;
}

// floats of one row of the tile in LDS: T + 1, odd for every even T, so that lane r reading [r][t] hits bank (r + t) mod 32
constexpr unsigned sos_lds_stride(unsigned T) { return T | 1; }

}  // namespace host
}  // namespace kofft
