// host_common.hip.h -- what every translation unit of libkofft_hip.so shares: the context, the planner-table cache,
// launch geometry and the size dispatch.  The kernels are instantiated per family in their own translation units
// (k_complex_*.hip, k_real_*.hip, k_stft.hip, k_nd.hip, ...) so that the library builds in parallel, and each of those units holds
// its family's checks, launchers, host-pointer wrappers (host_stage.hip.h) and extern "C" entry points of include/kofft_hip.h;
// kofft_hip.hip keeps the context's lifecycle and the host-only recipes.  gfx950 only; compiled with -ffp-contract=off.
#pragma once

#include "../../include/kofft_hip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "fft_big.hip.h"
#include "fft_persist.hip.h"
#include "fft_istft.hip.h"
#include "fft_regfile.hip.h"
#include "fft_split_wide.hip.h"
#include "fft_wg.hip.h"
#include "host_cache.h"
#include "host_layout.h"
#include "persist_walk.h"
#include "tables.h"

// ---------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------
#define KOFFT_BIG_PROBE_MAX 8  /* candidates of the intermediate's placement probe (big_probe_pick) */
// One cached chirp-Z parameter set (k_spectral_f32.hip): key = (n, m, bits of wr, wi, ar, ai), compared whole; d_small = [wpow: 2 m |
// apow: 2 n] floats, d_table = the n x ldc table once a call has taken the table route.
struct kofft_spectral_slot {
    std::vector<unsigned> key;
    void *d_small = nullptr;
    void *d_table = nullptr;
};
constexpr size_t kSpectralSlots = 4;  // a 4096 x 4096 chirp-Z table is 128 MiB
// One cached filterbank plan (k_mfcc_f32.hip): key = (bins, n_fft, num_mel), compared whole; d_plan = [ints | w] as
// kofft_tables::mel_plan_build lays them out, uploaded stream-ordered from `staged`, which lives as long as the slot.
struct kofft_mel_slot {
    std::vector<uint64_t> bins;
    size_t n_fft = 0, num_mel = 0;
    std::vector<int> staged;
    void *d_plan = nullptr;
};
constexpr size_t kMelSlots = 4;
// One cached set of pixel ranges of the log-scaled spectrogram render (k_spectrogram_f32.hip): key = the caller's bin -> pixel table,
// compared whole; d_start = bins + 1 values (kofft_tables::spec_ranges_build), uploaded stream-ordered from `staged`.
struct kofft_spec_slot {
    std::vector<uint32_t> table;
    std::vector<uint32_t> staged;
    void *d_start = nullptr;
};
constexpr size_t kSpecSlots = 4;
struct kofft_hip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t order_event = nullptr;  // kofft_hip_set_stream: orders the new stream after the old one
    int num_cus = 256;
    bool use_persist = true;  // KOFFT_HIP_NO_PERSIST=1 forces the generic kernels (A/B measurements, tests)
    bool istft_fused = true;  // KOFFT_HIP_ISTFT_FUSED=0: ISTFT always as inverse transforms + the overlap-add kernel
    bool dct_fused = true;    // kofft_hip_set_dct_fused(ctx, 0): DCT-II of every length through the composed route (mirror, fft_dev, post-pass; A/B, tests)
    bool hilbert_fused = true; // kofft_hip_set_hilbert_fused(ctx, 0): analytic signals of every length through the composed route (expand, fft_dev, mask, inverse fft_dev; A/B, tests)
    bool planar_fused = true; // kofft_hip_set_split_fused(ctx, 0): planar (split re / im) transforms of every length through the composed route (pack, fft_dev, unpack; A/B, tests)
    bool cepstrum_fused = true; // kofft_hip_set_cepstrum_fused(ctx, 0): real cepstra of every length through the composed route (expand, fft_dev, log-magnitude, inverse fft_dev, real parts; A/B, tests)
    bool convolve_fused = true; // kofft_hip_set_convolve_fused(ctx, 0): overlap-save convolutions of every block through the composed route (expand, fft_dev, multiply, inverse fft_dev, gather; A/B, tests)
    bool convolve_bank_fused = true; // kofft_hip_set_convolve_bank_fused(ctx, 0): filter-bank convolutions of every block through the composed route (expand and fft_dev once, then per filter multiply, inverse fft_dev, gather; A/B, tests)
    bool mdct_fused = true;   // kofft_hip_set_mdct_fused(ctx, 0): fast DCT-IV, MDCT and IMDCT of every length through the composed route (fold / pre-twiddle, fft_dev, post-twiddle; A/B, tests)
    int pfb_fused = 1;        // kofft_hip_set_pfb_fused: 1 the measured choice (pfb_use_fused), 0 polyphase filter-bank analysis and synthesis of every M through the composed route (fold into the scratch, fft_dev, prefix copy / completion, inverse fft_dev, real parts), 2 the fused kernels wherever they exist (A/B, tests)
    int mfcc_fused = 1;       // kofft_hip_set_mfcc_fused: 1 the measured choice (mfcc_use_fused), 0 every MFCC through the composed route (filterbank, log, direct DCT-II, column copy), 2 the fused kernel wherever it fits (A/B, tests)
    int frontend_fused = 1;   // kofft_hip_set_frontend_fused: 1 the measured choice (frontend_use_fused), 0 every audio-to-mel / MFCC call through the composed route (magnitudes into the scratch, then the mel / MFCC path), 2 the fused kernel wherever it fits (A/B, tests)
    int welch_fused = 1;      // kofft_hip_set_welch_fused: 1 the measured choice (welch_use_fused), 0 every Welch / cross-spectrum call through the composed route (one-sided frames into the scratch, then the sums), 2 the fused kernel wherever it exists (A/B, tests)
    int resample_tiled = 1;   // kofft_hip_set_resample_tiled: 1 the measured choice (resample_route), 0 polyphase resampling of every shape on the plain kernel (one thread per output, global loads), 2 the tiled kernel wherever its tables fit the LDS budget (the same bytes; A/B, tests)
    int sosfilt_tiled = 1;    // kofft_hip_set_sosfilt_tiled: 1 the measured choice (sosfilt_use_tiled), 0 IIR filtering of every shape on the plain kernel (one thread per row, global loads), 2 the tiled kernel wherever it exists (the same bytes; A/B, tests)
    bool spec_transpose = true; // kofft_hip_set_spectrogram_transpose(ctx, 0): the image layout of the spectrogram render with every lane storing its own bytes instead of the exchange through LDS (the same bytes; A/B, tests)
    bool direct_tiled = true; // kofft_hip_set_direct_tiled(ctx, 0): direct DCT / DST sums of every shape on the simple kernel (one lane per output; A/B, tests)
    bool dht_table_device = true; // kofft_hip_set_dht_table_device(ctx, 0): the Hartley table of a new length built on the host and uploaded instead of by dht_table_kernel (the same bytes; A/B, tests)
    int wavelet_fused = 1;    // kofft_hip_set_wavelet_fused: 1 the measured choice (wavelet_use_fused), 0 every multi-level call level by level, 2 the fused kernels wherever they fit (A/B, tests)
    int czt_route = 0;        // kofft_hip_set_czt_route: 0 by batch and by whether the table is there (czt_use_table), 1 every call on czt_recur_kernel<CZT_SUM>, 2 every call through a table and the direct kernels (A/B, tests)
    bool blue_persist = true; // KOFFT_HIP_BLUESTEIN_PERSIST=0: the one-launch Bluestein arm always as one workgroup per XPB transforms
    int persist_grid_pct = 0; // KOFFT_HIP_PERSIST_GRID_PCT: scale the persistent grids (measurements only)
    int persist_claim_pct = -1; // kofft_hip_set_persist_claim_pct: percent of the batch the kClaim persistent kernels hand out by claim, 0 .. 100 (-1: the configuration's; A/B, tests)
    unsigned *persist_claim_counters = nullptr;  // device: nine 128-byte lines, the claim words in the first ones and the arrival word in the last (fft_persist.hip.h, PersistClaim); zeroed at creation, every kClaim launch leaves them at zero
    int persist_walk_mode = kofft::host::kPersistWalkRule;  // kofft_hip_set_persist_walk: -1 a kClaim launch on the buffer its predecessor wrote walks the other way (persist_walk.h), 0 ascending and no kept zone (the kernel of round 8), 1 / 2 ascending / descending with the kept zone (A/B, tests)
    size_t persist_keep_bytes = kofft::host::kPersistKeepDefaultBytes;  // kofft_hip_set_persist_keep_bytes: the end of a kClaim walk that is stored with the default cache policy
    kofft::host::PersistWalkRecord persist_walk_last;  // what the last kClaim launch wrote and which way it walked (launch_persist_claim)
    unsigned long long persist_walk_launches = 0;      // kofft_hip_persist_walk_debug: kClaim launches so far, and the last one's plan
    kofft::host::PersistWalkPlan persist_walk_plan_last{false, 0};
    size_t persist_walk_batch_last = 0;
    int big_three_min = 22;    // KOFFT_HIP_BIG_THREE_MIN: smallest log2 n split into three factors
    bool small32 = true;       // KOFFT_HIP_SMALL32=0: f32 n = 32 on the thread-group kernel instead of one thread per transform (A/B)
    bool big_first11 = true;   // KOFFT_HIP_BIG_FIRST11=0: 2^21 as 2^10 x 2^11 with the one-tile-per-workgroup kernel for the 2^11 factor (A/B)
    bool big_narrow = true;    // KOFFT_HIP_BIG_NARROW=0: full-width tiles even when they leave CUs without a workgroup (A/B)
    bool big_persist = true;   // KOFFT_HIP_BIG_PERSIST=0: factors on the one-tile-per-workgroup kernel (A/B measurements)
    bool blue_fused = true;    // KOFFT_HIP_BLUESTEIN_FUSED=0: pointwise steps as separate kernels at every size
    bool blue_one_kernel = true;  // KOFFT_HIP_BLUESTEIN_ONE=0: two launches through a scratch even where one workgroup holds m points
    bool nd_transpose = true;  // KOFFT_HIP_ND_TRANSPOSE=0: long strided axes through the strided kernel
    bool nd_fused = true;      // KOFFT_HIP_ND_FUSED=0: 2-D c32 images with 1024 .. 4096-point rows through rows + two column-tile passes instead of the fused two passes (A/B)
    bool nd_two_pass = true;   // KOFFT_HIP_ND_TWO_PASS=0: power-of-two axes of 4096 .. 16384 points through the transposes instead of two column-tile passes (A/B)
    bool zero_copy = true;     // KOFFT_HIP_ZERO_COPY=0: small host calls through staged copies like large ones
    bool host_pipeline = true; // KOFFT_HIP_HOST_PIPELINE=0: host-pointer batches in one upload / kernel / download
    bool rfft14_wide = true;    // KOFFT_HIP_RFFT14_WIDE=0: rfft / irfft of 32768 reals on the generic kernel
    bool rfft13_persist = true; // KOFFT_HIP_RFFT13_PERSIST=0: rfft / irfft n = 16384 on the generic kernel
    int persist64 = 1;         // KOFFT_HIP_PERSIST64=0: c64 n = 4096 / 8192 on the generic kernel (A/B measurements)
    bool persist_small = true; // KOFFT_HIP_PERSIST_SMALL=0: n = 128, 256 on the generic kernels (A/B measurements)
                               // double-buffered one (measured, same box: c32 0.52-0.53 against 0.61-0.63, STFT 0.41 against 0.43)
    bool rfft_regfile_epi = true;  // KOFFT_HIP_RFFT_REGFILE_EPI=0: rfft of 65536 (f32) / 32768 (f64) reals as register-file transform + post-pass kernel (two passes) instead of one (A/B)
    bool use_regfile = true;   // KOFFT_HIP_REGFILE=0: c32 2^15 / c64 2^14 on the two-factor path instead of the register-file-resident kernel (A/B)
    bool use_split = true;     // KOFFT_HIP_SPLIT=0: n = 8192 on the block-synchronised persistent kernel instead of the wave-split one (A/B)
    std::string last_error;
    // planner caches: (kind, n) -> device table, every kind in TableKind (host_cache.h); read and filled by device_table / device_table_pair alone
    kofft::host::TableCache tables;
    // chirp-Z tables: most recently used first, at most kSpectralSlots; an evicted slot is freed after the stream is synchronised.
    // goertzel_coeff: the device-pointer Goertzel's coefficients (kGoertzelMaxFreqs floats), goertzel_last what it holds.
    // kofft_hip_destroy and kofft_hip_release_scratch drop all of it (spectral_drop)
    std::vector<kofft_spectral_slot> czt_slots;
    void *goertzel_coeff = nullptr;
    std::vector<float> goertzel_last;
    // filterbank plans: most recently used first, at most kMelSlots; dropped with the chirp-Z tables (mel_drop)
    std::vector<kofft_mel_slot> mel_slots;
    // pixel ranges of the log-scaled spectrogram render: most recently used first, at most kSpecSlots; dropped with the plans above
    std::vector<kofft_spec_slot> spec_slots;
    // staging for the host-pointer entry points: one device buffer, laid out by host_layout() (host_layout.h)
    kofft::host::DevBuf stage;
    // intermediate of the two-factor large-n path (fft_big.hip.h): `big_chunk` transforms at a time
    kofft::host::DevBuf big_tmp;
    bool big_row_pairs = true;       // KOFFT_HIP_BIG_ROW_PAIRS=0: c32 last factor one row per thread slot (8-row tiles) instead of row pairs (A/B)
    bool big_blocked = true;         // KOFFT_HIP_BIG_BLOCKED=0: natural layout of the two-factor intermediate (A/B)
    // placement probe of big_tmp (round 6, complex_impl.hip.h: big_probe_pick): candidates timed, figures of the last probe
    int big_probe = 5;               // KOFFT_HIP_BIG_PROBE: candidate allocations per probe (0 / 1: take what hipMalloc hands out)
    int big_probe_n = 0, big_probe_pick = -1;
    float big_probe_first_us[KOFFT_BIG_PROBE_MAX] = {}, big_probe_total_us[KOFFT_BIG_PROBE_MAX] = {};
    // small host-pointer calls (one frame, one transform): a pinned, device-mapped buffer the kernels read and write
    // directly over PCIe -- one launch and one synchronisation instead of two staged copies around them
    void *pinned = nullptr;      // host address
    void *pinned_dev = nullptr;  // the same memory as the device sees it
    size_t pinned_bytes = 0;
    kofft::host::DevBuf blue_tmp;  // zero-padded work buffer of the Bluestein arm
    kofft::host::DevBuf real_tmp;  // the inner complex transform of real / STFT lengths the fused kernels do not cover
    kofft::host::DevBuf rows_tmp;  // istft_parallel_rows on device pointers: the inverse transforms of the caller's (const) frames
    size_t scratch_chunk_bytes = kofft::host::kScratchChunkDefaultBytes;  // KOFFT_HIP_SCRATCH_CHUNK_MB (1 .. 512): the scratch of one pass of every chunk loop but the factor path's (scratch_chunk_rows, host_layout.h); the N-D transpose panels take twice this
    size_t big_chunk_bytes = size_t(512) << 20;  // KOFFT_HIP_BIG_CHUNK_MB; measured on config 5 with the persistent factor kernels: 128 MiB 14.7 ms, 256 13.0, 512 12.1, 1024 12.5, 2048 13.1
};

namespace kofft {
namespace host {

#define KOFFT_HIP_TRY(ctx, expr)                                                              \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);            \
            return KOFFT_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)

// The body of a route-switch setter (kofft_hip_set_*): a bool member takes value != 0, an int member the value itself, which must lie
// in [lo, hi].
template <class F>
inline int set_route(kofft_hip_ctx *ctx, F kofft_hip_ctx::*member, int value, int lo = INT_MIN, int hi = INT_MAX)
{
    if (!ctx) return KOFFT_ERR_NULL;
    if (value < lo || value > hi) return KOFFT_ERR_INVALID_VALUE;
    ctx->*member = static_cast<F>(value);  // (bool: value != 0)
    return KOFFT_OK;
}

inline bool is_pow2(size_t n) { return n != 0 && (n & (n - 1)) == 0; }
inline int ilog2(size_t n)
{
    int l = 0;
    while ((size_t(1) << l) < n) ++l;
    return l;
}

// The grid of a flat grid-stride kernel of 256 threads over `total` elements: one thread per element up to per_cu workgroups per CU
// (a tuning value of the family that calls), the kernel's stride loop takes the rest.
inline unsigned flat_blocks(const kofft_hip_ctx *ctx, size_t total, size_t per_cu)
{
    const size_t want = (total + 255) / 256, cap = (size_t)ctx->num_cus * per_cu;
    return (unsigned)(want < cap ? want : cap);
}

// The allocator of the table cache and the scratch buffers (host_cache.h).  A failed hipMalloc also leaves its error with the runtime,
// where the next launch's hipGetLastError would find it: taken away here.
struct HipAlloc {
    static const char *alloc(void **p, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) return nullptr;
        (void)hipGetLastError();
        return hipGetErrorString(e);
    }
    static const char *free(void *p)
    {
        const hipError_t e = hipFree(p);
        return e == hipSuccess ? nullptr : hipGetErrorString(e);
    }
};

// cached_table / cached_table_pair on device memory (P, Q: the tables' element types)
template <typename P, class Build>
int device_table(kofft_hip_ctx *ctx, TableKind kind, size_t n, size_t bytes, const char *label, const P **out, Build build)
{
    return cached_table<HipAlloc>(ctx, kind, n, bytes, label, out, build);
}
template <typename P, typename Q, class Build>
int device_table_pair(kofft_hip_ctx *ctx, TableKind kind_a, TableKind kind_b, size_t n, size_t bytes_a, size_t bytes_b, const char *label,
                      const P **out_a, const Q **out_b, Build build)
{
    return cached_table_pair<HipAlloc>(ctx, kind_a, kind_b, n, bytes_a, bytes_b, label, out_a, out_b, build);
}
// what most builders end with.  A synchronous copy: tables are built once per (context, n), never in a timed region
inline int upload_table(void *d, const void *host, size_t bytes, std::string &why)
{
    const hipError_t e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) return KOFFT_OK;
    why = hipGetErrorString(e);
    return KOFFT_ERR_HIP;
}

// The planner tables of one length, n >= 1: `entries` complex values filled by f32 / f64 (tables.h)
template <typename T>
int planner_table(kofft_hip_ctx *ctx, TableKind kind, size_t n, size_t entries, void (*f32)(size_t, float *), void (*f64)(size_t, double *),
                  const cpx<T> **out)
{
    const size_t vals = 2 * (entries ? entries : 1);
    return device_table(ctx, kind, n, vals * sizeof(T), "table upload", out, [&](void *d, std::string &why) {
        std::vector<T> host(vals);
        if constexpr (sizeof(T) == 4) f32(n, (float *)host.data());
        else f64(n, (double *)host.data());
        return upload_table(d, host.data(), vals * sizeof(T), why);
    });
}
// FftPlanner's twiddles (n / 2 entries), RfftPlanner's post-pass table (n entries), DctPlanner's (cos, sin) pairs (n; f32 only: dct.rs:6)
template <typename T>
int twiddle_table(kofft_hip_ctx *ctx, size_t n, const cpx<T> **out)
{
    return planner_table<T>(ctx, kind_for<T>(kTableTwF32), n, n / 2, kofft_tables::twiddles_f32, kofft_tables::twiddles_f64, out);
}
template <typename T>
int rfft_table(kofft_hip_ctx *ctx, size_t n, const cpx<T> **out)
{
    return planner_table<T>(ctx, kind_for<T>(kTableRfftF32), n, n, kofft_tables::rfft_table_f32, kofft_tables::rfft_table_f64, out);
}
inline int dct2_table(kofft_hip_ctx *ctx, size_t n, const cpx<float> **out)
{
    return planner_table<float>(ctx, kTableDct2, n, n, kofft_tables::dct2_table_f32, nullptr, out);
}
// the fast DCT-IV's twiddles of an even n: c at out[0 .. n/2), d at out[n/2 .. n)
inline int dct4_table(kofft_hip_ctx *ctx, size_t n, const cpx<float> **out)
{
    return planner_table<float>(ctx, kTableDct4Fast, n, n, kofft_tables::dct4_table_f32, nullptr, out);
}

constexpr size_t kZeroCopyMax = size_t(512) << 10;  // bytes per direction up to which a host call goes zero-copy
// (measured per-call latency, host memory: n = 64 31 -> 17 us, 1024 33 -> 20, 4096 36 -> 22, 65536 95 -> 79; 1 MiB: no gain)

inline int ensure_pinned(kofft_hip_ctx *ctx, size_t bytes)
{
    if (ctx->pinned_bytes >= bytes) return KOFFT_OK;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = ctx->pinned_dev = nullptr;
    ctx->pinned_bytes = 0;
    const size_t want = bytes < (size_t(1) << 20) ? (size_t(1) << 20) : bytes;
    if (hipHostMalloc(&ctx->pinned, want, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        ctx->pinned = nullptr;
        return KOFFT_ERR_ALLOC;
    }
    if (hipHostGetDevicePointer(&ctx->pinned_dev, ctx->pinned, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        return KOFFT_ERR_ALLOC;
    }
    ctx->pinned_bytes = want;
    return KOFFT_OK;
}

// grow-only device scratch: ensure(ctx, ctx->real_tmp, bytes), then ctx->real_tmp.p
inline int ensure(kofft_hip_ctx *ctx, DevBuf &buf, size_t bytes) { return ensure_buf<HipAlloc>(ctx, buf, bytes); }
// every device scratch buffer of a context and the pinned one go (kofft_hip_destroy, kofft_hip_release_scratch)
inline void drop_buffers(kofft_hip_ctx *ctx)
{
    for (DevBuf *b : {&ctx->stage, &ctx->big_tmp, &ctx->blue_tmp, &ctx->real_tmp, &ctx->rows_tmp}) release_buf<HipAlloc>(*b);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = ctx->pinned_dev = nullptr;
    ctx->pinned_bytes = 0;
}

// ---------------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------------
// threads per transform >= 8 (c64) / 16 (c32): every load / store instruction covers whole 128-byte lines per transform
// (A/B on one box: n = 32 c64 0.65 -> 0.79 of the roofline, n = 64 c32 0.64 -> 0.71, n = 128 c32 0.60 -> 0.70.)
constexpr int rl_for(int L) { return (L == 5 || L == 6) ? 2 : (L == 7 || L == 9) ? 3 : (L >= 13 ? 5 : 4); }
constexpr int block_for(int L)
{
    const int tpt = (1 << L) >> rl_for(L);
    return tpt > 256 ? tpt : 256;
}
template <typename T> constexpr int max_log2();
template <> constexpr int max_log2<float>() { return 14; }
template <> constexpr int max_log2<double>() { return 13; }

// hipFuncSetAttribute once per (kernel instance, device): `done` is a function-local static of the caller's template
// instance, one bit per device ordinal.  Later calls skip it, so `lds` must be the largest the kernel ever takes (a
// constant of the instance, or its maximum where the LDS depends on the call: launch_fwd_fused).
inline int set_dyn_lds_once(kofft_hip_ctx *ctx, std::atomic<unsigned long long> &done, const void *kern, size_t lds)
{
    const unsigned long long bit = 1ull << (ctx->device & 63);
    if (ctx->device < 64 && (done.load(std::memory_order_relaxed) & bit)) return KOFFT_OK;
    KOFFT_HIP_TRY(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (ctx->device < 64) done.fetch_or(bit, std::memory_order_relaxed);
    return KOFFT_OK;
}

// Points per thread of the one-workgroup-per-transform kernel at n = 8192 / 16384: 32 (half the threads, one exchange less)
// or 16.  Measured per kind on one box (tools/sweep.py, 4 against 5 in rl_for): 16 wins for every f64 kernel of 8192
// points (c64 +7 %, rfft64 n = 16384 +18 %, irfft64 +8 %) and for the f32 real-input kernels (rfft32 n = 16384 +22 %,
// 32768 +4 %); 32 wins for c32 16384 (+4 %) and STFT 16384 (+14 %); irfft32 does not care.
template <typename T, int EPI>
constexpr int rl_for_kind(int L)
{
    return (L >= 13 && (sizeof(T) == 8 || EPI == EPI_RFFT)) ? 4 : rl_for(L);
}

template <typename T, int L, int EPI, class IO, int BLOCK_OVERRIDE = 0>
int launch_wg(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    // (sub-transforms of the large-n path come with their own block size, computed for rl_for)
    constexpr int RL = BLOCK_OVERRIDE ? rl_for(L) : rl_for_kind<T, EPI>(L);
    constexpr int TPT0 = (1 << L) >> RL;
    // f64 from n = 512: one transform per workgroup down to a single wavefront (round 3, same box, 256 -> 64 / 128 threads: rfft64
    // n = 2048 0.62 -> 0.71, c64 2048 0.72 -> 0.75, c64 / rfft64 512 .. 1024 +2..4 %, irfft64 2048 0.63 -> 0.64..0.66; below
    // 512 and for f32 the results are mixed (+-4 %) and the workgroups stay at 256)
    constexpr int MINB = (sizeof(T) == 8 && L >= 9) ? 64 : 256;
    constexpr int BLOCK = BLOCK_OVERRIDE ? BLOCK_OVERRIDE : (TPT0 > MINB ? TPT0 : MINB);
    constexpr int TPT = (1 << L) >> RL;
    constexpr int XPB = BLOCK / TPT;
    constexpr size_t lds = lds_wg_bytes<T, wg_split_lds<T, L, EPI, IO>(), IO::kSlotMinor, XPB>(1 << L);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = fft_wg_kernel<T, L, RL, BLOCK, EPI, IO>;
    if (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        const int arc = set_dyn_lds_once(ctx, attr_done, reinterpret_cast<const void *>(kern), lds);
        if (arc) return arc;
    }
    const size_t blocks = (batch + XPB - 1) / XPB;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BLOCK), lds, ctx->stream, io, tw, batch);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// Persistent, prefetching kernels (fft_persist.hip.h): the streaming path for large batches.  Every workgroup walks the
// batch with a stride of the grid size and keeps the next transform's loads in flight while it computes.
// PersistCfg<L, IO> is the per-(size, policy) configuration, each value chosen by same-box A/B measurement:
//   BLOCK / RL      threads per workgroup, log2 of the points per thread (threads per transform = n >> RL)
//   MINW            waves per SIMD the kernel must fit (register budget); WG_PER_CU = workgroups launched per CU
//   kInvInLds       window samples / irfft table in one LDS copy per workgroup instead of registers
//   kTwLastInLds    the last pass reads its twiddles from an LDS copy of the table (frees 24..30 VGPRs)
//   kClaim          (default off) the end of the batch is handed out by claim; kClaimPct: how much of it, in percent
template <int L, class IO> struct PersistCfg;
template <class IO> struct PersistCfgBase {
    static constexpr int NBUF = 1, RL = 4;
    static constexpr bool kInvInLds = IO::kInvInLds, kTwLastInLds = false;
};
template <class IO> struct PersistCfg<13, IO> : PersistCfgBase<IO> { static constexpr int BLOCK = 512, MINW = 2, WG_PER_CU = 1; };
// c64 n = 8192 (round 3; n = 4096 below): 136 KiB of exchange buffer is one workgroup per CU either way; the generic kernel then runs its load,
// transform and store phases with nothing beside them.  Persistent with the next transform's loads in flight; table entries
// from global memory in every pass (kTwGlobal: no room for them in registers or LDS).
template <bool INV> struct PersistCfg<13, ComplexIO<double, INV>> {
    static constexpr int BLOCK = 512, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 1;
    static constexpr bool kInvInLds = false, kTwLastInLds = false, kTwGlobal = true;
};
template <bool INV> struct PersistCfg<12, ComplexIO<double, INV>> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 2;
    static constexpr bool kInvInLds = false, kTwLastInLds = false, kTwGlobal = true;
};
// (DEPTH, round 5 A/B: two transforms ahead for the n = 4096 kernels -- three register sets, 166 VGPRs -- measured without gain)
template <class IO> struct PersistCfg<12, IO> : PersistCfgBase<IO> { static constexpr int BLOCK = 256, MINW = 2, WG_PER_CU = 2, DEPTH = 1; };
// c32 n = 4096 (round 7): the last kClaimPct percent of the batch are claimed row by row instead of walked (fft_persist.hip.h,
// PersistClaim), so that a workgroup that falls behind leaves rows to the others; the table of fractions is in DESIGN.md 5.2.
// (round 8: 87 percent through two claim words; 25 was the largest share ONE word could hand out below its own rate)
template <bool INV> struct PersistCfg<12, ComplexIO<float, INV>> : PersistCfgBase<ComplexIO<float, INV>> {
    static constexpr int BLOCK = 256, MINW = 2, WG_PER_CU = 2, DEPTH = 1, kClaimPct = 87;
    static constexpr bool kClaim = true;
};
template <class IO> struct PersistCfg<11, IO> : PersistCfgBase<IO> { static constexpr int BLOCK = 256, MINW = 2, WG_PER_CU = 2; };
template <class IO> struct PersistCfg<10, IO> : PersistCfgBase<IO> {
    static constexpr int BLOCK = 256, MINW = IO::kLeanRegisters ? 3 : 2, WG_PER_CU = MINW;
};
// rfft 2048 (m = 1024, one wavefront per transform): with half the grid (PersistGrid below: fewer concurrent rows) a CU
// runs ONE wavefront per SIMD, and one transform of work is too short for the next one's loads to land: two ahead.
template <> struct PersistCfg<10, RfftIO<float>> : PersistCfgBase<RfftIO<float>> {
    static constexpr int BLOCK = 256, MINW = 2, WG_PER_CU = 2, DEPTH = 2;
};
template <> struct PersistCfg<10, StftIO> : PersistCfgBase<StftIO> {
    static constexpr int BLOCK = 256, MINW = 2, WG_PER_CU = 2, DEPTH = 1;
};
// stft_magnitudes runs the n-point COMPLEX transform of each real frame (visual/spectrogram.rs:52-76): twice STFT's butterflies for half
// its output -- compute-limited at every window; window in LDS and three workgroups per CU: n = 1024 0.210 -> 0.195 ms (config 4's stream)
template <> struct PersistCfg<10, StftMagIO> {
    // (the last pass's twiddles from an LDS copy -- no spill at three workgroups -- measured slower: 0.205 -> 0.220 ms)
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 3, WG_PER_CU = 3, DEPTH = 1;
    static constexpr bool kInvInLds = true, kTwLastInLds = false;
};
// irfft prefetches two row elements per output: the last pass reads its twiddles from LDS to stay inside 256 VGPRs
template <> struct PersistCfg<10, IrfftIO<float>> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 2, DEPTH = 1;
    static constexpr bool kInvInLds = true, kTwLastInLds = true;
};
template <> struct PersistCfg<11, IrfftIO<float>> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 2;
    static constexpr bool kInvInLds = true, kTwLastInLds = true;
};
// STFT n = 2048 / 4096 is compute-limited (more stages per point): with the window in LDS the kernel fits 3 waves/SIMD
// (158 VGPRs), measured +5.5 % / +3.5 % (the memory-limited complex kernel LOSES 4 % with a third workgroup per CU).
template <class IO> struct PersistCfgStftBig {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 3, WG_PER_CU = 3;
    static constexpr bool kInvInLds = true, kTwLastInLds = false;
};
// (round 4: 8 points per thread -- four passes, 104-107 registers, four wavefronts per SIMD -- measured 8 % slower at both sizes)
template <> struct PersistCfg<12, StftIO> : PersistCfgStftBig<StftIO> {};
template <> struct PersistCfg<11, StftIO> : PersistCfgStftBig<StftIO> {};
// (the magnitude kernels spill 21 / 11 registers at three workgroups per CU -- tools/kernel_regs.py -- and are still 13 % faster than at two:
// n = 2048 / 4096 0.219 / 0.226 against 0.250 / 0.254 ms)
template <> struct PersistCfg<12, StftMagIO> : PersistCfgStftBig<StftMagIO> {};
template <> struct PersistCfg<11, StftMagIO> : PersistCfgStftBig<StftMagIO> {};
// the row-aware heirs (fft_wg.hip.h, StftRowsOf) run their parents' configurations
template <> struct PersistCfg<10, StftRowsIO> : PersistCfg<10, StftIO> {};
template <> struct PersistCfg<11, StftRowsIO> : PersistCfg<11, StftIO> {};
template <> struct PersistCfg<12, StftRowsIO> : PersistCfg<12, StftIO> {};
template <> struct PersistCfg<10, StftMagRowsIO> : PersistCfg<10, StftMagIO> {};
template <> struct PersistCfg<11, StftMagRowsIO> : PersistCfg<11, StftMagIO> {};
template <> struct PersistCfg<12, StftMagRowsIO> : PersistCfg<12, StftMagIO> {};
// (the one-sided STFT, k_stft_onesided.hip: StftIO's arithmetic and registers, fewer stores)
template <> struct PersistCfg<10, StftHalfRowsIO> : PersistCfg<10, StftIO> {};
template <> struct PersistCfg<11, StftHalfRowsIO> : PersistCfg<11, StftIO> {};
template <> struct PersistCfg<12, StftHalfRowsIO> : PersistCfg<12, StftIO> {};
// rfft 8192 (m = 4096): window pairs in registers so that two workgroups (exchange buffer + post-pass table) fit a CU
template <> struct PersistCfg<12, RfftIO<float>> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 2;
    static constexpr bool kInvInLds = false, kTwLastInLds = false;
};
// rfft 16384 (m = 8192): one 512-thread workgroup per CU (exchange buffer 68 KiB + post-pass table 64 KiB)
template <> struct PersistCfg<13, RfftIO<float>> {
    static constexpr int BLOCK = 512, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 1;
    static constexpr bool kInvInLds = false, kTwLastInLds = false;
};
// irfft 16384 (m = 8192): the same, with the pre-pass table in LDS and every pass's twiddles from global memory
template <> struct PersistCfg<13, IrfftIO<float>> {
    static constexpr int BLOCK = 512, NBUF = 1, RL = 4, MINW = 2, WG_PER_CU = 1;
    static constexpr bool kInvInLds = true, kTwLastInLds = false, kTwGlobal = false;
};
// n = 64: 4 points per thread, 16 threads per transform, three passes of two stages
template <class IO> struct PersistCfg<6, IO> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 2, MINW = 4, WG_PER_CU = 4;
    static constexpr bool kInvInLds = IO::kInvInLds, kTwLastInLds = false;
};
// n = 256, 128: 8 points per thread, 32 / 16 threads per transform -> 2 / 4 transforms per wavefront
template <class IO> struct PersistCfg<8, IO> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 3, MINW = 4, WG_PER_CU = 4;
    static constexpr bool kInvInLds = IO::kInvInLds, kTwLastInLds = false;
};
template <class IO> struct PersistCfg<7, IO> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 3, MINW = 4, WG_PER_CU = 4;
    static constexpr bool kInvInLds = IO::kInvInLds, kTwLastInLds = false;
};
// n = 512: 8 points per thread so that a transform is still one wavefront (three passes of three stages)
template <class IO> struct PersistCfg<9, IO> {
    static constexpr int BLOCK = 256, NBUF = 1, RL = 3, MINW = 4, WG_PER_CU = 4;
    static constexpr bool kInvInLds = IO::kInvInLds, kTwLastInLds = false;
};

// Workgroups per CU actually launched.  The rfft kernels (misaligned 8200-byte output rows, an extra LDS round trip)
// stream better with FEWER concurrent rows once the batch no longer fits the 256 MiB Infinity Cache: measured at 4 GiB
// of input, n = 512 / 1024 / 2048: +6 % / +4 % / +4 % with half the grid (config 3: 3.49 -> 3.37 ms; n = 128 / 256: the
// persistent kernel only beats the generic one, by 10 %, with half the grid); at 512 MiB the
// 2048-point kernel loses 10 % with half the grid, the two smaller ones still gain.  STFT and complex want the full grid.
template <int L, class IO> struct PersistGrid {
    static int wg_per_cu(int base, size_t) { return base; }
};
// (with the group-wide stores of round 3 (fft_persist.hip.h) three workgroups beat two by 6 %)
template <> struct PersistGrid<6, RfftIO<float>> { static int wg_per_cu(int, size_t) { return 3; } };
template <> struct PersistGrid<7, RfftIO<float>> { static int wg_per_cu(int base, size_t) { return base / 2; } };
template <> struct PersistGrid<8, RfftIO<float>> { static int wg_per_cu(int base, size_t) { return base / 2; } };
template <> struct PersistGrid<9, RfftIO<float>> { static int wg_per_cu(int base, size_t) { return base / 2; } };
template <> struct PersistGrid<10, RfftIO<float>> {
    static int wg_per_cu(int base, size_t input_bytes) { return input_bytes > (size_t(1) << 30) ? base / 2 : base; }
};

// What the chip-resident launchers below end with: the kernel's LDS attribute (done: the CALLER's function-local static, one per kernel
// instance), the launch on `blocks` workgroups, its error.
template <class Kern, class IO, class TW>
int launch_resident(kofft_hip_ctx *ctx, std::atomic<unsigned long long> &done, Kern kern, size_t blocks, int block, size_t lds, const IO &io,
                    const TW *tw, size_t batch)
{
    const int arc = set_dyn_lds_once(ctx, done, reinterpret_cast<const void *>(kern), lds);
    if (arc) return arc;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(block), lds, ctx->stream, io, tw, batch);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

template <typename T, int L, int EPI, class IO>
int launch_persist_claim(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch);
template <typename T, int L, int EPI, class IO>
int launch_persist(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Cfg = PersistCfg<L, IO>;
    if constexpr (persist_claim<Cfg>::value) return launch_persist_claim<T, L, EPI>(ctx, io, tw, batch);
    else {
    constexpr int RL = Cfg::RL;
    constexpr int XPB = Cfg::BLOCK / ((1 << L) >> RL);
    constexpr size_t lds = (size_t)XPB * Cfg::NBUF * persist_slot_elems(L) * sizeof(cpx<T>) +
                           (Cfg::kInvInLds ? (size_t)(1 << L) * sizeof(typename IO::Inv) : 0) +
                           (EPI == EPI_RFFT ? (size_t)(1 << L) * sizeof(cpx<T>) : 0) +
                           (Cfg::kTwLastInLds ? (size_t)(1 << L) / 2 * sizeof(cpx<T>) : 0);
    static_assert(lds * Cfg::WG_PER_CU <= 160 * 1024, "LDS budget");
    static std::atomic<unsigned long long> attr_done{0};
    const size_t blocks = resident_blocks(ctx->num_cus, PersistGrid<L, IO>::wg_per_cu(Cfg::WG_PER_CU, batch * sizeof(cpx<T>) << L),
                                          ctx->persist_grid_pct, (batch + XPB - 1) / XPB);
    return launch_resident(ctx, attr_done, fft_persist_kernel<T, L, RL, EPI, IO, Cfg>, blocks, Cfg::BLOCK, lds, io, tw, batch);
    }
}

// The same for a kClaim configuration.  Rows [0, split) are walked as above, split a multiple of the grid's stride; rows [split, batch)
// are claimed through the context's claim words, which every launch leaves at zero (no reset here, nothing a captured graph's replay
// would miss: pointer and split are plain kernel arguments that depend on the batch alone).  They ride in the kernel's IO policy.
template <typename T, int L, int EPI, class IO>
int launch_persist_claim(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Cfg = PersistCfg<L, IO>;
    constexpr int RL = Cfg::RL;
    constexpr int XPB = Cfg::BLOCK / ((1 << L) >> RL);
    constexpr size_t lds = (size_t)XPB * Cfg::NBUF * persist_slot_elems(L) * sizeof(cpx<T>) + 16;  // + the words the claims travel through
    static_assert(lds * Cfg::WG_PER_CU <= 160 * 1024, "LDS budget");
    if (!ctx->persist_claim_counters) {
        ctx->last_error = "the context has no claim counters";
        return KOFFT_ERR_ALLOC;
    }
    using KIO = PersistClaimIO<IO>;  // the kernel's policy: `io` plus the hand-out's argument
    static std::atomic<unsigned long long> attr_done{0};
    // (no more workgroups than tiles of XPB rows: every workgroup's first walked row exists)
    const size_t blocks = resident_blocks(ctx->num_cus, PersistGrid<L, IO>::wg_per_cu(Cfg::WG_PER_CU, batch * sizeof(cpx<T>) << L),
                                          ctx->persist_grid_pct, (batch + XPB - 1) / XPB);
    const size_t stride = blocks * XPB;
    const size_t pct = ctx->persist_claim_pct < 0 ? (size_t)Cfg::kClaimPct : (ctx->persist_claim_pct > 100 ? 100 : (size_t)ctx->persist_claim_pct);
    size_t claimed = batch / 100 * pct + batch % 100 * pct / 100;
    if (claimed > (size_t(1) << 31)) claimed = size_t(1) << 31;  // (row offsets from split travel as 32-bit tickets)
    // (round 9) Direction and kept zone: persist_walk.h.  The context remembers the range this launch writes and the way it walks, for
    // the next one.  Mirror and keep_from are plain kernel arguments too, but they depend on the CALL HISTORY: a captured graph replays
    // the directions it was captured with, whatever ran on the buffer in between -- correct by construction (any direction computes the
    // same rows), and a graph of an even number of calls on one buffer keeps alternating across its replays.
    const size_t row_bytes = sizeof(cpx<T>) << L, bytes = batch * row_bytes;
    const uintptr_t in_lo = reinterpret_cast<uintptr_t>(io.in), out_lo = reinterpret_cast<uintptr_t>(io.out);
    const kofft::host::PersistWalkPlan plan = kofft::host::persist_walk_plan(ctx->persist_walk_mode, ctx->persist_walk_last, in_lo, bytes, out_lo,
                                                                             bytes, batch, row_bytes, ctx->persist_keep_bytes);
    ctx->persist_walk_last = kofft::host::PersistWalkRecord{out_lo, bytes, plan.mirror};
    ctx->persist_walk_plan_last = plan;
    ctx->persist_walk_batch_last = batch;
    ++ctx->persist_walk_launches;
    const KIO kio{io, PersistClaim{ctx->persist_claim_counters, (batch - claimed) / stride * stride, plan.keep_from, plan.mirror ? 1u : 0u}};
    return launch_resident(ctx, attr_done, fft_persist_kernel<T, L, RL, EPI, KIO, Cfg>, blocks, Cfg::BLOCK, lds, kio, tw, batch);
}

// The wave-split kernel (fft_split.hip.h): one workgroup per CU, one s_barrier per transform.
template <typename T, int LA, int LB, class IO>
int launch_split(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Gm = SplitGeom<LA, LB>;
    constexpr size_t lds = 2 * (size_t)Gm::N * sizeof(cpx<T>) + 16;  // (+ the two counters of KOFFT_SPLIT_COUNTERS)
    static_assert(lds <= 160 * 1024, "LDS budget");
    static std::atomic<unsigned long long> attr_done{0};
    const size_t blocks = resident_blocks(ctx->num_cus, 1, ctx->persist_grid_pct, batch);
    return launch_resident(ctx, attr_done, fft_split_persist_kernel<T, LA, LB, IO>, blocks, Gm::TPT, lds, io, tw, batch);
}


// n = 2^14 with 32 points per thread (fft_split_wide.hip.h): 512 threads, one workgroup per CU, 128-byte runs both ways
template <typename T, int LA, int LB, int QB0, class IO>
int launch_split_wide(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Gm = SplitWideGeom<LA, LB, QB0>;
    constexpr size_t lds = split_wide_lds_bytes<Gm>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    static std::atomic<unsigned long long> attr_done{0};
    const size_t blocks = resident_blocks(ctx->num_cus, (int)((160 * 1024) / lds), ctx->persist_grid_pct, batch);
    return launch_resident(ctx, attr_done, fft_split_wide_persist_kernel<T, LA, LB, QB0, IO>, blocks, Gm::TPT, lds, io, tw, batch);
}

// c32 n = 2^15 / c64 n = 2^14: the whole transform in the CU's register file (fft_regfile.hip.h), one 1024-thread workgroup per CU
template <typename T, int LA, int LB, int QB0, class IO>
int launch_regfile(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Gm = RfGeom<T, LA, LB, QB0>;
    constexpr size_t lds = regfile_lds_bytes<Gm, T>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    static std::atomic<unsigned long long> attr_done{0};
    const size_t blocks = resident_blocks(ctx->num_cus, 1, ctx->persist_grid_pct, batch);
    return launch_resident(ctx, attr_done, fft_regfile_persist_kernel<T, LA, LB, QB0, IO>, blocks, Gm::TPT, lds, io, tw, batch);
}

// rfft of 2^15 reals: the same kernel with the post-pass as its epilogue (two instances: with / without a row window)
template <typename T, int LA, int LB, int QB0, class IO>
int launch_split_wide_rfft(kofft_hip_ctx *ctx, const IO &io, const cpx<T> *tw, size_t batch)
{
    using Gm = SplitWideGeom<LA, LB, QB0>;
    constexpr size_t lds = split_wide_lds_bytes<Gm>();
    const bool win = io.window != nullptr;
    auto kern = win ? fft_split_wide_persist_kernel<T, LA, LB, QB0, IO, EPI_RFFT, true> : fft_split_wide_persist_kernel<T, LA, LB, QB0, IO, EPI_RFFT, false>;
    static std::atomic<unsigned long long> attr_done[2] = {{0}, {0}};
    const size_t blocks = resident_blocks(ctx->num_cus, (int)((160 * 1024) / lds), ctx->persist_grid_pct, batch);
    return launch_resident(ctx, attr_done[win ? 1 : 0], kern, blocks, Gm::TPT, lds, io, tw, batch);
}

template <typename T, int N, int EPI, class IO>
int launch_small(kofft_hip_ctx *ctx, const IO &io, size_t batch, const cpx<T> *tw = nullptr)
{
    constexpr int kSmallBlock = small_block_threads<N, IO>();
    const size_t blocks = (batch + kSmallBlock - 1) / kSmallBlock;
    if (blocks > 0x7fffffffULL) return KOFFT_ERR_UNSUPPORTED;
    constexpr size_t lds = small_lds_bytes<T, N, IO>();
    auto kern = fft_small_kernel<T, N, EPI, IO>;
    if (lds > 64 * 1024) {
        static std::atomic<unsigned long long> attr_done{0};
        const int arc = set_dyn_lds_once(ctx, attr_done, reinterpret_cast<const void *>(kern), lds);
        if (arc) return arc;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kSmallBlock), lds, ctx->stream, io, tw, batch);
    KOFFT_HIP_TRY(ctx, hipGetLastError());
    return KOFFT_OK;
}

// adjacent columns / rows per workgroup: 128-byte segments (16 x c32, 8 x c64) when the LDS budget allows
// (measured, c32: 2^15..2^19 0.19 -> 0.225 of the roofline, 2^22..2^24 0.12 -> 0.15)
template <typename T>
constexpr int big_xpb() { return sizeof(T) == 4 ? 16 : 8; }
// LDS_CAP: bytes of exchange buffer a workgroup may use -- 80 KiB where two workgroups share a CU (the one-tile-per-
// workgroup kernels), 128 KiB for the persistent kernels (one workgroup per CU): c32 tiles of 2^10-point sub-transforms
// are then 16 columns = 128-byte segments instead of 8 = 64.
template <typename T, class IO, int LS, size_t LDS_CAP = 80 * 1024>
constexpr int big_block()
{
    const int tpt = (1 << LS) >> rl_for(LS);
    int xpb = big_xpb<T>();
    // (f64: at most 512 threads -- two register sets of 16 values are 128 VGPRs, a 1024-thread block has 128 in all)
    while (xpb > 1 && (xpb * tpt > (sizeof(T) == 8 ? 512 : 1024) || (size_t)xpb * (1 << LS) * 8 > LDS_CAP)) xpb /= 2;
    int block = xpb * tpt;
    if (block < 64) block = 64;
    return block;
}

// Run the n-point transform described by `io` (n a power of two >= 1) over `batch` units.
template <typename T, int EPI, class IO>
int dispatch(kofft_hip_ctx *ctx, const IO &io, size_t n, size_t batch)
{
    if (batch == 0) return KOFFT_OK;
    const int L = ilog2(n);
    if (L > max_log2<T>()) return KOFFT_ERR_UNSUPPORTED;
    switch (L) {
    case 0:
        if constexpr (IO::kLen1) return launch_small<T, 1, EPI>(ctx, io, batch);
        else return KOFFT_ERR_UNSUPPORTED;  // (never: the policy's callers handle n = 1 themselves)
    case 1: return launch_small<T, 2, EPI>(ctx, io, batch);
    case 2: return launch_small<T, 4, EPI>(ctx, io, batch);
    case 3: return launch_small<T, 8, EPI>(ctx, io, batch);
    case 4: return launch_small<T, 16, EPI>(ctx, io, batch);
    default: break;
    }
    const cpx<T> *tw = nullptr;
    int rc = twiddle_table<T>(ctx, n, &tw);
    if (rc) return rc;
    // n = 32 in f32: still one thread per transform (64 data registers), IO staged through LDS like the small sizes
    if constexpr (sizeof(T) == 4 && !IO::kSlotMinor) if (L == 5 && ctx->small32) return launch_small<T, 32, EPI>(ctx, io, batch, tw);
    if constexpr (sizeof(T) == 8 && EPI == EPI_STORE && io_split_ok<IO>::value && IO::kPersist) {
        if (L == 13 && ctx->use_persist && ctx->persist64 && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 13, EPI>(ctx, io, tw, batch);
        // n = 4096: two 256-thread workgroups per CU, same box 0.64-0.65 -> 0.67-0.68; n = 2048 measured too: no change (0.70), left
        if (L == 12 && ctx->use_persist && ctx->persist64 && batch >= (size_t)ctx->num_cus * 8) return launch_persist<T, 12, EPI>(ctx, io, tw, batch);
    }
    if constexpr (sizeof(T) == 4 && IO::kPersist) if (ctx->use_persist) {
        // streaming sizes: enough transforms to give every resident workgroup several iterations
        if constexpr (EPI == EPI_STORE && io_split_ok<IO>::value) {
            if (L == 14 && ctx->use_split && batch >= (size_t)ctx->num_cus * 4) return launch_split_wide<T, 7, 7, 2>(ctx, io, tw, batch);
        }
        if constexpr (EPI == EPI_STORE && IO::kPersistMaxLog2 >= 13) {
            if constexpr (io_split_ok<IO>::value) {
                if (L == 13 && ctx->use_split && batch >= (size_t)ctx->num_cus * 4) return launch_split<T, 7, 6>(ctx, io, tw, batch);
            }
            if (L == 13 && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 13, EPI>(ctx, io, tw, batch);
            if (L == 12 && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 12, EPI>(ctx, io, tw, batch);
        }
        if constexpr (EPI == EPI_STORE && io_pairs_in_wave<IO>::value) {
            if (L == 14 && ctx->use_split && ctx->rfft14_wide && batch >= (size_t)ctx->num_cus * 4) return launch_split_wide<T, 7, 7, 2>(ctx, io, tw, batch);
            if (L == 13 && ctx->rfft13_persist && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 13, EPI>(ctx, io, tw, batch);
        }
        if constexpr (EPI == EPI_RFFT) {
            if (L == 14 && ctx->use_split && ctx->rfft14_wide && batch >= (size_t)ctx->num_cus * 4)
                return launch_split_wide_rfft<T, 7, 7, 2>(ctx, io, tw, batch);
            if (L == 13 && ctx->rfft13_persist && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 13, EPI>(ctx, io, tw, batch);
        }
        if constexpr (EPI == EPI_RFFT || (EPI == EPI_STORE && IO::kPersistMaxLog2 == 12)) {
            if (L == 12 && batch >= (size_t)ctx->num_cus * 4) return launch_persist<T, 12, EPI>(ctx, io, tw, batch);
        }
        if (L == 11 && batch >= (size_t)ctx->num_cus * 16) return launch_persist<T, 11, EPI>(ctx, io, tw, batch);
        if (L == 10 && batch >= (size_t)ctx->num_cus * 32) return launch_persist<T, 10, EPI>(ctx, io, tw, batch);
        if (L == 9 && batch >= (size_t)ctx->num_cus * 64) return launch_persist<T, 9, EPI>(ctx, io, tw, batch);
        if (ctx->persist_small && io.group_rows_ok()) {
            if constexpr (IO::kPersistMinLog2 <= 8)
                if (L == 8 && batch >= (size_t)ctx->num_cus * 128) return launch_persist<T, 8, EPI>(ctx, io, tw, batch);
            if constexpr (IO::kPersistMinLog2 <= 7)
                if (L == 7 && batch >= (size_t)ctx->num_cus * 256) return launch_persist<T, 7, EPI>(ctx, io, tw, batch);
            if constexpr (IO::kPersistMinLog2 <= 6)
                if (L == 6 && batch >= (size_t)ctx->num_cus * 512) return launch_persist<T, 6, EPI>(ctx, io, tw, batch);
        }
    }
    switch (L) {
    // lane-over-lines policies (strided axes): as many adjacent lines per workgroup as big_block allows (128-byte segments)
#define KOFFT_CASE(LL) \
    case LL: return launch_wg<T, LL, EPI, IO, (IO::kSlotMinor ? big_block<T, IO, LL>() : 0)>(ctx, io, tw, batch);
        KOFFT_CASE(5)
        KOFFT_CASE(6)
        KOFFT_CASE(7)
        KOFFT_CASE(8)
        KOFFT_CASE(9)
        KOFFT_CASE(10)
        KOFFT_CASE(11)
        KOFFT_CASE(12)
        KOFFT_CASE(13)
    case 14:
        if constexpr (sizeof(T) == 4) return launch_wg<T, 14, EPI>(ctx, io, tw, batch);
        else return KOFFT_ERR_UNSUPPORTED;
#undef KOFFT_CASE
    default: return KOFFT_ERR_UNSUPPORTED;
    }
}

template <typename T> constexpr int max_log2_big() { return 26; }
// complex lengths fft_dev takes: powers of two up to 2^26, anything else (Bluestein, m = next_pow2(2n-1)) up to 2^25
inline bool complex_len_ok(size_t n) { return n <= (size_t(1) << (is_pow2(n) ? 26 : 25)); }
// inner lengths the fused real / STFT kernels cover (one workgroup per transform); the rest is composed (real_impl.hip.h)
template <typename T> inline bool fused_len_ok(size_t m) { return is_pow2(m) && m <= (size_t(1) << max_log2<T>()); }

// hann(win_len), cached per context like a planner table: stft_magnitudes' window, one signal or rows
inline int hann_table(kofft_hip_ctx *ctx, size_t win_len, const float **out)
{
    return device_table(ctx, kTableHann, win_len, win_len * sizeof(float), "stft_magnitudes window upload", out, [&](void *d, std::string &why) {
        std::vector<float> w(win_len);
        kofft_tables::hann_f32(win_len, w.data());
        return upload_table(d, w.data(), win_len * sizeof(float), why);
    });
}

// ---- what one translation unit defines and another calls -----------------------------------------------------------------------
// Only that: a function that nothing outside its own unit calls is not declared here and has internal linkage there
// (tests/test_abi_symbols.py counts the files that mention each name between the two marks).
// [cross-unit declarations: begin]
template <typename T>
int fft_dev(kofft_hip_ctx *ctx, const T *d_in, T *d_out, size_t n, size_t batch, int inverse);  // k_complex_f32/f64.hip
template <typename T>
int fft_axis2_dev(kofft_hip_ctx *ctx, T *d_data, int LT, int I, size_t blocks, int inverse);  // k_big_f32/f64.hip: ndfft's long axes in two passes
bool fft2d_fused_ok(const kofft_hip_ctx *ctx, size_t rows, size_t cols);                      // k_nd_fused.hip: shapes the two-pass 2-D route takes
int fft2d_fused_c32(kofft_hip_ctx *ctx, float *d_data, size_t rows, size_t cols, int inverse);  // ... rows + 2 column stages, then one column-tile pass
template <typename T>
int fft_big_windowed_dev(kofft_hip_ctx *ctx, const T *d_in, T *d_out, const T *d_window, size_t m, size_t batch);  // k_big_f32/f64.hip: factor path, window in the first load
int stft_bluestein_dev(kofft_hip_ctx *ctx, const float *d_signal, size_t len, const float *d_window, size_t n, size_t start0, size_t hop,
                       float *d_out, size_t count, bool *done);  // k_blue_f32.hip (complex_impl.hip.h)
// k_direct_f32.hip: dct::dct1..4 (family 0) / dst::dst1..4 (family 1), the direct sums, with their argument checks
constexpr size_t kDirectMaxN = 4096;  // the longest row: the n x n table is 64 MiB there
int direct_dev(kofft_hip_ctx *ctx, int family, int type, const float *d_in, float *d_out, size_t n, size_t batch);
// k_direct_f32.hip: the +0-seeded sums out[b][k] = sum_i x[b][i] * table[i][k], i < n, k < nk, on direct_tiled_kernel<DIR_ZERO> /
// direct_simple_kernel<DIR_ZERO> (direct_use_tiled(ctx, nk, batch)); table: n rows of direct_ldc(nk) floats
int direct_zero_sums(kofft_hip_ctx *ctx, const float *d_in, float *d_out, const float *table, size_t n, size_t nk, size_t batch);
void spectral_drop(kofft_hip_ctx *ctx);  // k_spectral_f32.hip: frees every chirp-Z slot and the Goertzel coefficient buffer; the caller has synchronised the stream
// k_mfcc_f32.hip: cepstrum::mel_filterbank / mfcc with the edges as an input (mfcc_impl.hip.h), with their argument checks; they
// return before the edge sizes (num_mel == 0, num_coeffs == 0) touch anything
constexpr size_t kMelMaxFft = size_t(1) << 24;  // (k - a) as f32 is exact below it
constexpr size_t kMfccFusedMaxMel = 128;        // the fused kernel's log-mel columns: 256 bytes of LDS per filter and workgroup
int mel_filterbank_dev(kofft_hip_ctx *ctx, const float *d_mags, float *d_energies, size_t n_fft, size_t rows, const uint64_t *bins,
                       size_t num_mel);
int mfcc_dev(kofft_hip_ctx *ctx, const float *d_mags, float *d_coeffs, size_t n_fft, size_t rows, const uint64_t *bins, size_t num_mel,
             size_t num_coeffs);
void mel_drop(kofft_hip_ctx *ctx);  // frees every plan; the caller has synchronised the stream
// the device plan [seg | live | w] of (bins, n_fft, num_mel) from the context's cache, built and uploaded stream-ordered on a miss
int get_mel_plan(kofft_hip_ctx *ctx, const uint64_t *bins, size_t n_fft, size_t num_mel, const int **out);
// k_spectrogram_f32.hip: visual::spectrogram's colour helpers (spectrogram_impl.hip.h)
constexpr size_t kSpecMaxBins = size_t(1) << 24;
// the device ranges [start[p], start[p + 1]) of a checked log_scale_bins table, from the context's cache (uploaded stream-ordered on a miss)
int get_spec_ranges(kofft_hip_ctx *ctx, const uint32_t *pix_of_bin, size_t bins, const uint32_t **out);
void spec_drop(kofft_hip_ctx *ctx);  // frees every range table; the caller has synchronised the stream
// k_frontend_f32.hip: magnitudes of frames [f0, f0 + nf) of each of nrows rows (f0 != 0: one row), dense at d_mags, no maximum; no
// checks (framed_produce's leaf for FRAMES_MAGS)
int mags_piece(kofft_hip_ctx *ctx, const float *d_signal, size_t nrows, size_t len, size_t row_stride, const float *d_win, size_t win_len,
               size_t hop, size_t f0, size_t nf, float *d_mags);
int stft_mag_dev(kofft_hip_ctx *ctx, const float *d_samples, size_t len, size_t win_len, size_t hop, float *d_mags,
                 size_t frames, float *d_max);  // k_stft.hip
// k_stft_rows.hip: the three families over `rows` signals (row r at + r * row_stride, one window, `frames` frames per row).
// *_check: the argument checks alone, before the context or a device is touched; host_form adds stft()'s frame-count check.
int stft_rows_check(bool host_form, bool mags, size_t rows, size_t len, size_t row_stride, size_t win_len, size_t hop, size_t frames);
int stft_mag_rows_dev(kofft_hip_ctx *ctx, const float *d_samples, size_t rows, size_t len, size_t row_stride, size_t win_len, size_t hop,
                      float *d_mags, size_t frames, float *d_max);
int istft_rows_check(size_t rows, size_t frames, size_t win_len, size_t hop, size_t out_len, size_t scratch_len, int mode);
// (mode 2 with keep_frames only) half: d_frames holds bins 0 .. win_len/2 of every frame, rows * frames * (win_len/2 + 1) complex; the
// walk's copy into the context's scratch is then the Hermitian completion (expand_half, k_stft_onesided.hip)
int istft_rows_dev(kofft_hip_ctx *ctx, float *d_frames, size_t rows, size_t frames, const float *d_window, size_t win_len, size_t hop,
                   float *d_output, size_t out_len, float *d_scratch, size_t scratch_len, int mode, bool keep_frames, bool half = false);
size_t composed_chunk(const kofft_hip_ctx *ctx, size_t win_len, size_t count);  // transforms per pass through at most ctx->scratch_chunk_bytes of scratch
// k_stft_rows.hip, for every family that cuts rows into frames.  What a framed call reads: `rows` signals cut into `frames` frames each, the flat index t = row * frames + frame.  framed_src is
// the one place that fills it: a null d_window becomes hann_table's (on the context: its only use of ctx)
struct FramedSrc {
    const float *signal, *win;
    size_t rows, len, row_stride /* 0 when rows == 1 */, win_len, hop, frames;
    bool kernels;  // the rows kernels cover win_len (fused_len_ok); otherwise stft_rows_composed
};
int framed_src(kofft_hip_ctx *ctx, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len,
               size_t hop, size_t frames, FramedSrc *src);
// Frames [t0, t0 + nt) of the flat index, dense at dst, as win_len complex values (FRAMES_FULL; composed lengths only), bins
// 0 .. win_len/2 (FRAMES_HALF) or the magnitudes of bins 0 .. win_len/2 - 1 without a maximum (FRAMES_MAGS; win_len >= 2).  The rows
// kernels run per rectangle of the chunk (frame_cut.h) through the two leaves below; the composed lengths go through
// stft_rows_composed -- into dst for FRAMES_FULL, otherwise into `spec` (nt * win_len complex, the caller's) and a per-element tail.
enum FramedForm { FRAMES_FULL, FRAMES_HALF, FRAMES_MAGS };
int framed_produce(kofft_hip_ctx *ctx, const FramedSrc &s, FramedForm form, size_t t0, size_t nt, void *dst, cpx<float> *spec);
// k_stft_onesided.hip: the one-sided STFT's kernels on frames [f0, f0 + nf) of each of nrows rows (f0 != 0: one row), dense at d_out; no checks
// (framed_produce's leaf for FRAMES_HALF)
int stft_onesided_piece(kofft_hip_ctx *ctx, const float *d_signal, size_t nrows, size_t len, size_t row_stride, const float *d_window,
                        size_t win_len, size_t hop, size_t f0, size_t nf, float *d_out);
// dst[t][k] = src[t][k] for k <= win_len/2, conj(src[t][win_len - k]) above: nt frames of win_len/2 + 1 bins -> nt frames of win_len
int expand_half(kofft_hip_ctx *ctx, const float *d_half, float *d_full, size_t nt, size_t win_len);
// [cross-unit declarations: end]

// the input side of a StftRowsOf policy (row_stride: 0 when rows == 1)
template <class IO>
inline void fill_rows_io(IO &io, const float *d_signal, size_t rows, size_t len, size_t row_stride, const float *d_window, size_t win_len,
                         size_t hop, size_t frames)
{
    io.signal = d_signal;
    io.window = d_window;
    io.out = nullptr;
    io.len = len;
    io.hop = hop;
    io.start0 = 0;
    io.n = (int)win_len;
    io.frames = frames;
    io.row_stride = rows > 1 ? row_stride : 0;
    io.frames32 = rows * frames < (size_t(1) << 31) ? (unsigned)frames : 0u;
}
template <class IO> inline void fill_rows_io(IO &io, const FramedSrc &s)
{
    fill_rows_io(io, s.signal, s.rows, s.len, s.row_stride, s.win, s.win_len, s.hop, s.frames);
}

}  // namespace host
}  // namespace kofft
