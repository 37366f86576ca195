// sosfilt_impl.hip.h -- batched IIR filtering of float rows by a cascade of biquads: scipy.signal.sosfilt's
// recurrence, bit for bit the definition of include/kofft_hip.h.  Per row, section s (ascending) and sample t (ascending, or
// descending with the reverse flag), with the section's input v (the previous section's output, x for s = 0) and state (z0, z1):
//   y  = (b0 * v) + z0
//   z0 = ((b1 * v) - (a1 * y)) + z1
//   z1 = (b2 * v) - (a2 * y)
// every product and sum one rounded f32 operation; the translation unit is built with -ffp-contract=off.  A rounded recurrence cannot
// be cut along time, so a row is walked by one lane and the parallelism is across rows.  A kernel instance holds NS <= kSosGroup
// sections: the state in 2 NS VGPRs, the 5 NS coefficients wave-uniform (scalar loads, SGPRs); a longer cascade runs further launches
// in place over `out` (a cascade is a composition).  Two kernels, the same operations per sample:
//  * PLAIN (every shape): sosfilt_plain_kernel, one thread per row over a flat grid, the thread walks its row in global memory
//    (lanes a row apart: every load and store of a wave touches 64 cache lines).
//  * TILED: sosfilt_tiled_kernel, one wavefront (a workgroup of 64 threads) per kSosRows rows, walked tile by tile along time.  A tile
//    of 64 rows x T samples is fetched with the lanes running along time (4-byte loads, 128 contiguous bytes per row: rows are only
//    4-byte aligned) and laid into LDS with a row stride of T + 1 floats; lane r then walks [r][0 .. len) -- bank (r + t) mod 32, no
//    conflict -- writes y back into the same slot, and the wave stores the tile the way it was fetched.  The other waves of the SIMD
//    (8448 bytes of LDS per wave: sixteen per CU) cover a wave's copies with their walks.  Lanes exchange data through LDS only across __syncthreads(), which for a
//    one-wave workgroup is the wavefront's fence and barrier; nothing relies on lockstep execution.  A tile never touches a sample
//    outside [0, nx) of its row or a row beyond `rows`: the short last tile and the partial last wave are masked in the fetch, the walk
//    and the store (sos_tile_in, sos_tile_out).
#pragma once

#include "host_common.hip.h"
#include "sosfilt_plan.h"

namespace kofft {

struct SosShape {
    size_t rows, nx;
    size_t sections;  // of the whole cascade: the state of a row is sections * 2 floats
    size_t first;     // the first section of this launch
    int reverse;
};

// the coefficients of NS sections (a0 is not read: the contract demands 1.0f)
template <int NS>
struct SosCoef {
    float b0[NS], b1[NS], b2[NS], a1[NS], a2[NS];
};

template <int NS>
__device__ __forceinline__ void sos_load_coef(SosCoef<NS> &c, const float *__restrict__ sos)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        c.b0[s] = sos[6 * s];
        c.b1[s] = sos[6 * s + 1];
        c.b2[s] = sos[6 * s + 2];
        c.a1[s] = sos[6 * s + 4];
        c.a2[s] = sos[6 * s + 5];
    }
}

// one sample through the NS sections: the definition, in its association
template <int NS>
__device__ __forceinline__ float sos_step(const SosCoef<NS> &c, float (&z0)[NS], float (&z1)[NS], float v)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float y = (c.b0[s] * v) + z0[s];
        z0[s] = ((c.b1[s] * v) - (c.a1[s] * y)) + z1[s];
        z1[s] = (c.b2[s] * v) - (c.a2[s] * y);
        v = y;
    }
    return v;
}

// the state of this launch's sections of one row: zi null is +0
template <int NS>
__device__ __forceinline__ void sos_load_state(float (&z0)[NS], float (&z1)[NS], const float *zi, size_t row, const SosShape &s)
{
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        z0[k] = zi ? zi[(row * s.sections + s.first + k) * 2] : 0.0f;
        z1[k] = zi ? zi[(row * s.sections + s.first + k) * 2 + 1] : 0.0f;
    }
}

template <int NS>
__device__ __forceinline__ void sos_store_state(const float (&z0)[NS], const float (&z1)[NS], float *zf, size_t row, const SosShape &s)
{
    if (!zf) return;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        zf[(row * s.sections + s.first + k) * 2] = z0[k];
        zf[(row * s.sections + s.first + k) * 2 + 1] = z1[k];
    }
}

// x and out may be the same buffer, zi and zf too: neither pair is __restrict__.  A thread reads sample t before it writes it and
// reads its row's state before the walk, writes it after.
template <int NS>
__global__ __launch_bounds__(256) void sosfilt_plain_kernel(const float *x, const float *__restrict__ sos, const float *zi, float *zf, float *out,
                                                            const SosShape s)
{
    SosCoef<NS> c;
    sos_load_coef<NS>(c, sos + 6 * s.first);
    const bool reverse = s.reverse != 0;
    for (size_t row = (size_t)blockIdx.x * host::kSosPlainThreads + threadIdx.x; row < s.rows; row += (size_t)gridDim.x * host::kSosPlainThreads) {
        float z0[NS], z1[NS];
        sos_load_state<NS>(z0, z1, zi, row, s);
        const float *xr = x + row * s.nx;
        float *orow = out + row * s.nx;
        for (size_t i = 0; i < s.nx; ++i) {
            const size_t t = host::sos_walk_at(i, s.nx, reverse);
            orow[t] = sos_step<NS>(c, z0, z1, xr[t]);
        }
        sos_store_state<NS>(z0, z1, zf, row, s);
    }
}

// Element j of a lane's share of a tile copy: row (lane / T) + (64 / T) * j of the wave's rows, sample lane % T of the tile (k = lane +
// 64 j in host::sos_tile_elem's count): the lanes run along time, 64 / T rows per load or store instruction.  t_ok: the lane's sample
// lies inside the tile (every lane's in a full tile).  A wave with all its 64 rows (wave-uniform) needs no test per element: the lanes
// past a short tile's end sit the copy out, and their LDS slots are neither walked nor stored.  The loops are rolled eight elements
// at a time: unrolled over the whole tile, the 64-bit offsets of all its elements are held in registers across the walk and spill.
__device__ __forceinline__ void sos_tile_in(float *lane_lds, const float *p, const float *safe, size_t copy_step, unsigned lds_step,
                                            unsigned count, unsigned r0, unsigned rp, unsigned nrows, bool all_rows, bool t_ok)
{
    if (all_rows) {
        if (t_ok) {
#pragma unroll 8
            for (unsigned j = 0; j < count; ++j) lane_lds[j * lds_step] = p[j * copy_step];
        }
    } else {
        // The last wave of a batch.  An element that does not exist loads the tile's first sample instead (`safe`: row row0, sample
        // tl * T, always there) and keeps +0: every load is unconditional, so the eight of a round are in flight together.
#pragma unroll 8
        for (unsigned j = 0; j < count; ++j) {
            const bool ok = t_ok && r0 + rp * j < nrows;
            const float v = *(ok ? p + j * copy_step : safe);
            lane_lds[j * lds_step] = ok ? v : 0.0f;
        }
    }
}

__device__ __forceinline__ void sos_tile_out(float *q, const float *lane_lds, size_t copy_step, unsigned lds_step, unsigned count, unsigned r0,
                                             unsigned rp, unsigned nrows, bool all_rows, bool t_ok)
{
    if (all_rows) {
        if (t_ok) {
#pragma unroll 8
            for (unsigned j = 0; j < count; ++j) q[j * copy_step] = lane_lds[j * lds_step];
        }
    } else {
#pragma unroll 8
        for (unsigned j = 0; j < count; ++j) {
            const float v = lane_lds[j * lds_step];
            if (t_ok && r0 + rp * j < nrows) q[j * copy_step] = v;
        }
    }
}

// PREFETCH (a measurement build only): the next tile is fetched into T registers before the walk and lies in flight
// during it, instead of the plain copy into LDS that leaves the overlap to the other waves of the SIMD.
template <int NS, bool PREFETCH>
__global__ __launch_bounds__(64) void sosfilt_tiled_kernel(const float *x, const float *__restrict__ sos, const float *zi, float *zf, float *out,
                                                           const SosShape s)
{
    constexpr unsigned T = host::kSosTile, R = host::kSosRows, S = host::sos_lds_stride(T);
    constexpr unsigned PER = T;       // elements of a tile per lane: R * T / 64
    constexpr unsigned RP = 64 / T;   // rows per copy instruction
    static_assert(R == 64 && T <= 64 && 64 % T == 0, "one lane per row, whole rows per copy instruction");
    __shared__ float tile[R * S];
    const unsigned lane = threadIdx.x;
    unsigned r0, t0;
    host::sos_tile_elem(lane, T, &r0, &t0);
    SosCoef<NS> c;
    sos_load_coef<NS>(c, sos + 6 * s.first);
    const bool reverse = s.reverse != 0;
    const size_t ngroups = host::sos_row_groups(s.rows), ntiles = host::sos_tiles(s.nx, T);
    const size_t lane_off = (size_t)r0 * s.nx + t0, copy_step = (size_t)RP * s.nx;
    float *const lane_lds = tile + r0 * S + t0;
    float *const mine_row = tile + lane * S;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const size_t row0 = g * R;
        const unsigned nrows = host::sos_group_rows(g, s.rows);
        const bool mine = lane < nrows;
        float z0[NS], z1[NS];
        if (mine) {
            sos_load_state<NS>(z0, z1, zi, row0 + lane, s);
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) z0[k] = z1[k] = 0.0f;
        }
        float pre[PREFETCH ? PER : 1];
        // the samples of tile `tl` that exist; the others are +0 and are never stored
        auto fetch = [&](size_t tl) {
            const unsigned len = host::sos_tile_len(tl, s.nx, T);
            const float *p = x + row0 * s.nx + tl * T + lane_off;
#pragma unroll
            for (unsigned j = 0; j < PER; ++j) pre[j] = (r0 + RP * j < nrows && t0 < len) ? p[j * copy_step] : 0.0f;
        };
        if (PREFETCH) fetch(host::sos_tile_at(0, ntiles, reverse));
        for (size_t step = 0; step < ntiles; ++step) {
            const size_t tl = host::sos_tile_at(step, ntiles, reverse);
            const unsigned len = host::sos_tile_len(tl, s.nx, T);
            const bool all_rows = nrows == R, t_ok = t0 < len;
            const size_t at = row0 * s.nx + tl * T + lane_off;
            if (PREFETCH) {
#pragma unroll
                for (unsigned j = 0; j < PER; ++j) lane_lds[j * RP * S] = pre[j];
            } else {
                sos_tile_in(lane_lds, x + at, x + (at - lane_off), copy_step, RP * S, PER, r0, RP, nrows, all_rows, t_ok);
            }
            __syncthreads();  // the tile is in LDS for the lanes that walk it
            if (PREFETCH && step + 1 < ntiles) fetch(host::sos_tile_at(step + 1, ntiles, reverse));
            if (mine) {
                if (len == T && !reverse) {  // (a full tile: constant LDS offsets)
#pragma unroll 8
                    for (unsigned i = 0; i < T; ++i) mine_row[i] = sos_step<NS>(c, z0, z1, mine_row[i]);
                } else if (len == T) {
#pragma unroll 8
                    for (unsigned i = 0; i < T; ++i) mine_row[T - 1 - i] = sos_step<NS>(c, z0, z1, mine_row[T - 1 - i]);
                } else {
                    for (unsigned i = 0; i < len; ++i) {
                        const unsigned t = (unsigned)host::sos_walk_at(i, len, reverse);
                        mine_row[t] = sos_step<NS>(c, z0, z1, mine_row[t]);
                    }
                }
            }
            __syncthreads();  // every row's outputs are in LDS for the lanes that store them
            sos_tile_out(out + at, lane_lds, copy_step, RP * S, PER, r0, RP, nrows, all_rows, t_ok);
            __syncthreads();  // the tile has been read before the next one overwrites it
        }
        if (mine) sos_store_state<NS>(z0, z1, zf, row0 + lane, s);
    }
}

// ---- the scan along time (kofft_hip_sosfilt_scan_f32) ------------------------------------------------------------
// A row is cut into C chunks of `chunk` samples (sosfilt_plan.h); the definition of include/kofft_hip.h in three launches per pass of
// at most kSosGroup sections:
//  1. sosfilt_scan_walk_kernel<NS, false> walks every chunk but a row's last from the +0 state and keeps its final state p_c in the state
//     scratch (no sample is stored); D = 2 NS further lanes walk `chunk` samples of +0 from the unit states and leave the columns of
//     the transition matrix M behind the states.
//  2. sosfilt_scan_carry_kernel<NS> runs Z_{c+1} = M Z_c + p_c along every row, one lane per state component, in the definition's order
//     of sums, and overwrites p_c with Z_{c+1}.
//  3. sosfilt_scan_walk_kernel<NS, true> walks every chunk from its true state Z_c (all of them from the scratch), stores the samples, and the lane of
//     a row's last chunk stores zf.
// The walk kernel is the tiled kernel over "virtual rows": a wavefront owns 64 consecutive (row, chunk) pairs, one per lane, and walks
// them in tiles of T samples through LDS with the same copies, stride and sos_step.  A tile slot holds walk step k * T + t of the
// lane's chunk whatever the direction, so the walk in LDS always ascends; with the reverse flag the copies run down the addresses.
// Where the 64 chunks are full ones of one row (wave-uniform), they lie `chunk` samples apart and the copies use one constant step;
// otherwise -- a wave across two rows, a short last chunk, the end of the batch, the unit-state lanes -- every element's address and
// length come from a table of the wave's 64 virtual rows in LDS.  No copy touches an element outside walk steps [0, len) of a chunk.
struct SosScanShape {
    size_t rows, nx;
    size_t sections;  // of the whole cascade
    size_t first;     // the first section of this pass
    size_t chunk;     // samples per chunk: a multiple of kSosTile
    size_t chunks;    // C = sos_scan_chunks(nx, chunk)
    int reverse;
};

template <int NS, bool STORE>
__global__ __launch_bounds__(64) void sosfilt_scan_walk_kernel(const float *x, const float *__restrict__ sos, const float *zi, float *zf, float *out,
                                                               float *st, const SosScanShape s)
{
    constexpr unsigned T = host::kSosTile, R = host::kSosRows, S = host::sos_lds_stride(T);
    constexpr unsigned PER = T, RP = 64 / T, D = 2 * NS;
    static_assert(R == 64 && T <= 64 && 64 % T == 0, "one lane per virtual row, whole rows per copy instruction");
    __shared__ float tile[R * S];
    __shared__ unsigned long long v_at[R];   // the element of walk step 0 of every virtual row of the wave
    __shared__ unsigned long long v_len[R];  // its samples; 0: nothing to copy (past the end of the batch, a unit-state lane)
    const unsigned lane = threadIdx.x;
    unsigned r0, t0;
    host::sos_tile_elem(lane, T, &r0, &t0);
    SosCoef<NS> c;
    sos_load_coef<NS>(c, sos + 6 * s.first);
    const bool reverse = s.reverse != 0;
    const size_t per = STORE ? s.chunks : s.chunks - 1;  // virtual rows a row: the first walk leaves the last chunk out
    const size_t ndata = s.rows * per, nv = STORE ? ndata : ndata + D;
    const size_t ngroups = host::sos_row_groups(nv);
    const size_t ntiles = host::sos_tiles(s.nx < s.chunk ? s.nx : s.chunk, T);
    float *const lane_lds = tile + r0 * S + t0;
    float *const mine_row = tile + lane * S;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const size_t v0 = g * R, v = v0 + lane;
        const bool data = v < ndata;
        size_t row = 0, ck = 0, len = 0, at = 0;
        float z0[NS], z1[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) z0[k] = z1[k] = 0.0f;
        if (data) {
            unsigned long long rr, cc;
            host::sos_scan_vrow(v, per, &rr, &cc);
            row = rr;
            ck = cc;
            len = host::sos_scan_len(ck, s.nx, s.chunk);
            at = host::sos_scan_at(row, ck, 0, s.nx, s.chunk, reverse);
            if (STORE) {
                // Chunk 0 of a row cut into several chunks takes Z_0 from the copy the carry kernel left in the scratch, not from zi: zf may
                // be zi, and the lane of the row's last chunk -- in another wavefront, at any time -- stores zf.  With one chunk a row the
                // lane that reads zi is the lane that writes zf.
                const float *from = s.chunks == 1 ? (zi ? zi + (row * s.sections + s.first) * 2 : nullptr)
                                                  : st + (ck == 0 ? host::sos_scan_z0_slot(row, s.rows, s.chunks, D) : row * (s.chunks - 1) + ck - 1) * D;
                if (from) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        z0[k] = from[2 * k];
                        z1[k] = from[2 * k + 1];
                    }
                }
            }
        } else if (!STORE && v < nv) {  // column v - ndata of the transition matrix: the unit state over `chunk` samples of +0
            const unsigned j = (unsigned)(v - ndata);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                z0[k] = j == 2u * k ? 1.0f : 0.0f;
                z1[k] = j == 2u * k + 1 ? 1.0f : 0.0f;
            }
        }
        const size_t walk_len = data ? len : (!STORE && v < nv ? s.chunk : 0);
        // wave-uniform: 64 full chunks of one row
        const size_t row_a = v0 / per, c_a = v0 - row_a * per;
        const bool uniform = v0 + R <= ndata && c_a + R <= per && host::sos_scan_len(c_a + R - 1, s.nx, s.chunk) == s.chunk;
        const size_t at_u = uniform ? host::sos_scan_at(row_a, c_a + r0, t0, s.nx, s.chunk, reverse) : 0;
        const size_t cstep = (size_t)RP * s.chunk;
        v_at[lane] = at;
        v_len[lane] = data ? len : 0;
        __syncthreads();  // the table is in LDS for the lanes that copy
        for (size_t k = 0; k < ntiles; ++k) {
            const size_t k0 = k * T;
            if (uniform) {
                const float *p = reverse ? x + (at_u - k0) : x + (at_u + k0);
                if (reverse) {
#pragma unroll 8
                    for (unsigned j = 0; j < PER; ++j) lane_lds[j * RP * S] = *(p - j * cstep);
                } else {
#pragma unroll 8
                    for (unsigned j = 0; j < PER; ++j) lane_lds[j * RP * S] = p[j * cstep];
                }
            } else {
                // An element that does not exist loads x[0] instead (always there) and keeps +0: every load is unconditional, so the eight
                // of a round are in flight together, as in sos_tile_in.
#pragma unroll 8
                for (unsigned j = 0; j < PER; ++j) {
                    const unsigned r = r0 + RP * j;
                    const size_t step = k0 + t0, a = v_at[r];
                    const bool ok = step < v_len[r];
                    const float val = x[ok ? (reverse ? a - step : a + step) : 0];
                    lane_lds[j * RP * S] = ok ? val : 0.0f;
                }
            }
            __syncthreads();  // the tile is in LDS for the lanes that walk it
            const unsigned wl = host::sos_scan_tile_len(walk_len, k, T);
            if (wl == T) {
#pragma unroll 8
                for (unsigned i = 0; i < T; ++i) {
                    const float y = sos_step<NS>(c, z0, z1, mine_row[i]);
                    if (STORE) mine_row[i] = y;
                }
            } else {
                for (unsigned i = 0; i < wl; ++i) {
                    const float y = sos_step<NS>(c, z0, z1, mine_row[i]);
                    if (STORE) mine_row[i] = y;
                }
            }
            __syncthreads();  // every chunk's outputs are in LDS for the lanes that store them; the tile has been read
            if (STORE) {
                if (uniform) {
                    float *q = reverse ? out + (at_u - k0) : out + (at_u + k0);
                    if (reverse) {
#pragma unroll 8
                        for (unsigned j = 0; j < PER; ++j) *(q - j * cstep) = lane_lds[j * RP * S];
                    } else {
#pragma unroll 8
                        for (unsigned j = 0; j < PER; ++j) q[j * cstep] = lane_lds[j * RP * S];
                    }
                } else {
#pragma unroll 8
                    for (unsigned j = 0; j < PER; ++j) {
                        const unsigned r = r0 + RP * j;
                        const size_t step = k0 + t0, a = v_at[r];
                        const float val = lane_lds[j * RP * S];
                        if (step < v_len[r]) out[reverse ? a - step : a + step] = val;
                    }
                }
                __syncthreads();  // the tile has been stored before the next one overwrites it
            }
        }
        if (STORE) {
            if (data && ck == s.chunks - 1 && zf) {
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    zf[(row * s.sections + s.first + k) * 2] = z0[k];
                    zf[(row * s.sections + s.first + k) * 2 + 1] = z1[k];
                }
            }
        } else if (v < nv) {  // slot v: p_c of a data lane, a column of M of a unit-state lane
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                st[v * D + 2 * k] = z0[k];
                st[v * D + 2 * k + 1] = z1[k];
            }
        }
        __syncthreads();  // the table has been read before the next group overwrites it
    }
}

// The carry: Z_{c+1}[i] = ((((M[i][0] Z_c[0]) + (M[i][1] Z_c[1])) + ..) + (M[i][J - 1] Z_c[J - 1])) + p_c[i], J = 2 (i / 2) + 2, for
// c = 0 .. C - 2 of every row.  Lane i of a group of D lanes holds row i of M and component i of the state; the lanes of a group read
// one another's component with a wavefront shuffle (every lane of the wave executes every shuffle: the triangular sum is a select, not a
// branch), 64 / D rows a wavefront.  The p_c of the next kScanAhead chunks are loaded before the current ones are consumed, so no step of the
// recurrence waits for a load it has just issued; Z_{c+1} overwrites p_c, which was read kScanAhead or more steps earlier.  The kernel
// also copies Z_0 (zi, or +0) into the row's own slot behind the matrix: the storing walk reads it there, because with zf == zi the
// wavefront of a row's last chunk may store zf before the wavefront of its chunk 0 has started.
constexpr unsigned kScanAhead = 16;

template <int NS>
__global__ __launch_bounds__(64) void sosfilt_scan_carry_kernel(float *st, const float *zi, const SosScanShape s)
{
    constexpr unsigned D = 2 * NS, RPW = 64 / D, U = kScanAhead;
    const unsigned lane = threadIdx.x, sub = lane / D, i = lane - sub * D;
    const unsigned src0 = (sub < RPW ? sub : RPW - 1) * D;  // (the idle lanes of a wave whose D does not divide 64 shuffle with the last group)
    const unsigned J = 2 * (i / 2) + 2;
    const size_t per = s.chunks - 1;  // >= 1
    const float *const mt = st + s.rows * per * D;
    float m[D];
#pragma unroll
    for (unsigned j = 0; j < D; ++j) m[j] = mt[j * D + i];
    const size_t nblocks = (s.rows - 1) / RPW + 1;
    for (size_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const size_t row = b * RPW + sub;
        const bool active = sub < RPW && row < s.rows;
        float *const p = st + (active ? row : 0) * per * D + i;  // (an idle lane neither loads nor stores)
        float z = active && zi ? zi[(row * s.sections + s.first) * 2 + i] : 0.0f;
        if (active) st[host::sos_scan_z0_slot(row, s.rows, s.chunks, D) * D + i] = z;  // Z_0 for the storing walk, which zf == zi may overwrite
        float cur[U], nxt[U];
#pragma unroll
        for (unsigned u = 0; u < U; ++u) cur[u] = active ? p[(u < per ? u : per - 1) * D] : 0.0f;
        for (size_t c0 = 0; c0 < per; c0 += U) {
#pragma unroll
            for (unsigned u = 0; u < U; ++u) {
                const size_t cn = c0 + U + u;
                nxt[u] = active ? p[(cn < per ? cn : per - 1) * D] : 0.0f;
            }
#pragma unroll
            for (unsigned u = 0; u < U; ++u) {
                float acc = 0.0f;
#pragma unroll
                for (unsigned j = 0; j < D; ++j) {
                    const float prod = m[j] * __shfl(z, (int)(src0 + j), 64);
                    acc = j == 0 ? prod : (j < J ? acc + prod : acc);
                }
                const float zn = acc + cur[u];
                const bool in = c0 + u < per;  // wave-uniform
                z = in ? zn : z;
                if (in && active) p[(c0 + u) * D] = z;
            }
#pragma unroll
            for (unsigned u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
}

}  // namespace kofft
