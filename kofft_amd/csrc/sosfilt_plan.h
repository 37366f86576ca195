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
constexpr unsigned kSosTile = 32;   // T: samples per tile (KOFFT_HIP_SOSFILT_TILE): 16, 32 or 64
constexpr bool kSosPrefetch = false;  // the next tile prefetched into registers (sosfilt_impl.hip.h) measured no faster
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

// ---- the scan along time (sosfilt_scan) ----
// A row of nx samples is cut into C = sos_scan_chunks chunks of `chunk` samples (a multiple of the tile) counted in walk order: chunk c
// holds walk steps [c * chunk, min(nx, (c + 1) * chunk)) of the row, so the short chunk is the last one walked in both directions.  A
// "virtual row" v of a batch cut into `per_row` chunks a row is chunk v % per_row of row v / per_row; a wavefront owns kSosRows
// consecutive virtual rows.  Walk step i of a chunk lies in tile i / T of that chunk: the tile grid starts at the chunk's first walked
// sample, which with the reverse flag is its highest address.

// chunks of a row of nx samples (nx >= 1, chunk >= 1)
KOFFT_SOS_HD unsigned long long sos_scan_chunks(unsigned long long nx, unsigned long long chunk) { return (nx - 1) / chunk + 1; }

// virtual row v -> (row, chunk) with per_row >= 1 chunks a row
KOFFT_SOS_HD void sos_scan_vrow(unsigned long long v, unsigned long long per_row, unsigned long long *row, unsigned long long *c)
{
    *row = v / per_row;
    *c = v - *row * per_row;
}

// samples of chunk c < sos_scan_chunks(nx, chunk): `chunk`, or what is left of the row in the last one.  Never 0.
KOFFT_SOS_HD unsigned long long sos_scan_len(unsigned long long c, unsigned long long nx, unsigned long long chunk)
{
    const unsigned long long left = nx - c * chunk;
    return left < chunk ? left : chunk;
}

// the element of the batch (row * nx + sample) that walk step i < sos_scan_len of chunk c of row `row` touches: ascending from sample
// c * chunk, or with the reverse flag descending from sample nx - 1 - c * chunk
KOFFT_SOS_HD unsigned long long sos_scan_at(unsigned long long row, unsigned long long c, unsigned long long i, unsigned long long nx,
                                            unsigned long long chunk, bool reverse)
{
    const unsigned long long step = c * chunk + i;
    return row * nx + (reverse ? nx - 1 - step : step);
}

// samples of tile k of a chunk of `len` samples: T, what is left in the chunk's last tile, 0 past it
KOFFT_SOS_HD unsigned sos_scan_tile_len(unsigned long long len, unsigned long long k, unsigned T)
{
    if (k * T >= len) return 0;
    const unsigned long long left = len - k * T;
    return left < T ? (unsigned)left : T;
}

// Floats of the state scratch of one pass over `rows` rows of C chunks with a state of D = 2 * sections components: one slot of D floats
// for each of the C - 1 seams of a row (slot row * (C - 1) + c: p_c after the first walk, Z_{c+1} after the carry), then D slots for
// the transition matrix, slot j holding column j (M[0 .. D)[j]), then one slot a row for Z_0 (sos_scan_z0_slot): the carry kernel copies
// zi there, so that the storing walk never reads zi, which zf may alias.
KOFFT_SOS_HD unsigned long long sos_scan_state_floats(unsigned long long rows, unsigned long long C, unsigned D)
{
    return (rows * C + D) * D;
}
KOFFT_SOS_HD unsigned long long sos_scan_z0_slot(unsigned long long row, unsigned long long rows, unsigned long long C, unsigned D)
{
    return rows * (C - 1) + D + row;
}

// The measured rule behind kofft_hip_sosfilt_scan_chunk (profiles/sosfilt_scan_bench.txt).  Two costs pull apart: the
// carry is sequential over the nx / chunk seams of a row, and the walks need rows * nx / chunk / 64 wavefronts to fill the device.  Rows
// of 2^20 samples and fewer (64 x 2^20, 4096 x 48 000, 65 536 x 3000) measured fastest at 1024 at every section count; rows of 2^24 and
// 28.8 M samples (16 and 1 of them) at 2048, except the single row through 8 and 12 sections, which measured faster at 4096 outside the
// spread (16 x 2^24 through 8 sections: 4096 faster by 3 % in one run, a tie in another).  Between 2^20 and 2^24 samples a row nothing was measured: the line is drawn at 2^22.  Never below kSosScanMinChunk: shorter
// chunks cost accuracy with poles close to the unit circle.
constexpr unsigned long long kSosScanMinChunk = 1024;
constexpr unsigned long long kSosScanLongRow = 1ull << 22;
KOFFT_SOS_HD unsigned long long sos_scan_chunk_rule(unsigned long long rows, unsigned long long nx, unsigned long long sections)
{
    if (nx < kSosScanLongRow) return kSosScanMinChunk;
    return rows == 1 && sections >= 8 ? 4 * kSosScanMinChunk : 2 * kSosScanMinChunk;
}

}  // namespace host
}  // namespace kofft
