// ubench_copy4.hip -- the persistent / prefetching copy of ubench_copy3.hip (copy_persist: nt loads and stores, next step prefetched,
// grid = 2 x CUs), varying what that tool held fixed: the bytes of one workgroup step, and which row a workgroup takes in a round.
// Development tool (round 8): decides whether the 4096-point c32 kernel's row-to-workgroup mapping or step footprint, and the single
// word of its claim hand-out, cost bandwidth.  2 GiB in, 2 GiB out, and the in-place form (same buffer).
//
//   cell      step per workgroup                       row of block b in round k (grid G)
//   base      32 KiB, 256 threads, 8-byte lanes        k*G + b                                   (the kernel today)
//   rot8      32 KiB, 256 threads                      k*G + 8*(b/8) + ((b%8) + (b/8)) % 8       (an XCD's rows cover all residues mod 8)
//   xcd8th    32 KiB, 256 threads                      k*G + (b%8)*(G/8) + b/8                   (an XCD streams one contiguous eighth)
//   pair64    64 KiB, 512 threads, one workgroup/CU    k*G' + b, G' = G/2
//   pair64w   as pair64, 16-byte lanes
//   c64shape  64 KiB, 256 threads, 16-byte lanes       k*G + b                                   (the c64 kernel's shape: the control)
//   claimS@P  base's step; the last P percent of the rows are not walked but claimed, one step ahead, by one lane through an LDS word,
//             from S counter words (S = 1: one word; S = 8: one word per blockIdx % 8 on its own 128-byte line, each over one contiguous
//             eighth of the claimed rows; a workgroup whose shard is empty walks on to the next one and never returns; S = 32: four words
//             per XCD; claim8i: shard s owns the claimed rows = s mod 8 instead of a contiguous eighth)
// (blocks past the last full group of 8 keep b: both maps are permutations of [0, G) for any G)
//
// Cells are interleaved in one process over ROUNDS rounds of REPS launches; per cell: the median and minimum of its round medians, and
// the box's spread = the largest (max - min) of any one cell's round medians.  Every out-of-place cell is checked once against the input.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

enum { MAP_BASE, MAP_ROT8, MAP_XCD8TH };

template <int MAP>
__host__ __device__ inline unsigned row_map(unsigned b, unsigned G)
{
    const unsigned full = G / 8 * 8;
    if (MAP == MAP_BASE || b >= full) return b;
    if (MAP == MAP_ROT8) return 8 * (b / 8) + ((b % 8) + (b / 8)) % 8;
    return (b % 8) * (G / 8) + b / 8;
}

template <int BLOCK, int LW, int STEPB>
struct Mover {
    using V = typename std::conditional<LW == 8, f2v, f4v>::type;
    static constexpr int NL = STEPB / (BLOCK * LW);
    static __device__ __forceinline__ void load(V *r, const char *in, unsigned row, int t)
    {
        const V *p = reinterpret_cast<const V *>(in + (size_t)row * STEPB);
#pragma unroll
        for (int u = 0; u < NL; ++u) r[u] = __builtin_nontemporal_load(p + t + BLOCK * u);
    }
    static __device__ __forceinline__ void store(const V *r, char *out, unsigned row, int t)
    {
        V *p = reinterpret_cast<V *>(out + (size_t)row * STEPB);
#pragma unroll
        for (int u = 0; u < NL; ++u) __builtin_nontemporal_store(r[u], p + t + BLOCK * u);
    }
};

// (no __restrict__: the in-place form passes one buffer twice)
template <int BLOCK, int MINW, int LW, int STEPB, int MAP>
__global__ __launch_bounds__(BLOCK, MINW) void copy_walk(const char *in, char *out, unsigned nrows)
{
    using M = Mover<BLOCK, LW, STEPB>;
    const int t = threadIdx.x;
    const unsigned G = gridDim.x;
    unsigned row = row_map<MAP>(blockIdx.x, G);
    if (row >= nrows) return;
    typename M::V cur[M::NL], nxt[M::NL];
    M::load(cur, in, row, t);
    for (;;) {
        const unsigned nrow = row + G;
        const bool more = nrow < nrows;
        if (more) M::load(nxt, in, nrow, t);
        M::store(cur, out, row, t);
        if (!more) break;
#pragma unroll
        for (int u = 0; u < M::NL; ++u) cur[u] = nxt[u];
        row = nrow;
    }
}

// The claim hand-out of fft_persist_kernel without the transform: rows [0, split) walked (split a multiple of the grid), rows
// [split, nrows) claimed one step ahead.  counters: SHARDS words 32 unsigned apart; the host zeroes them before every launch.
constexpr unsigned kLine = 32;  // unsigned per 128-byte line
constexpr size_t kCounterBytes = 33 * 128;
template <int SHARDS, bool INTERLEAVE = false>
struct Claimer {
    unsigned *counters;
    unsigned split, nrows, shard, visited;
    __device__ __forceinline__ unsigned lo(unsigned s) const { return split + (nrows - split) / SHARDS * s; }
    __device__ __forceinline__ unsigned hi(unsigned s) const { return s + 1 == SHARDS ? nrows : lo(s + 1); }
    // a row, or ~0u when this shard is exhausted
    __device__ __forceinline__ unsigned row_of(unsigned ticket) const
    {
        if (INTERLEAVE) {  // shard s owns the claimed rows = s (mod SHARDS)
            const unsigned long long r = (unsigned long long)split + (unsigned long long)ticket * SHARDS + shard;
            return r < nrows ? (unsigned)r : ~0u;
        }
        const unsigned r = lo(shard) + ticket;
        return r < hi(shard) ? r : ~0u;
    }
    __device__ __forceinline__ unsigned fetch() { return atomicAdd(counters + shard * kLine, 1u); }
    // after a failed claim: the next shards, one after the other, waiting for each answer; nrows when all of them are exhausted
    __device__ unsigned walk_on()
    {
        while (++visited < SHARDS) {
            shard = (shard + 1) % SHARDS;
            const unsigned r = row_of(fetch());
            if (r != ~0u) return r;
        }
        return nrows;
    }
    __device__ unsigned claim_now()
    {
        if (visited >= SHARDS) return nrows;
        const unsigned r = row_of(fetch());
        return r != ~0u ? r : walk_on();
    }
};

template <int SHARDS, bool INTERLEAVE>
__global__ __launch_bounds__(256, 2) void copy_claim(const char *in, char *out, unsigned nrows, unsigned split, unsigned *counters)
{
    using M = Mover<256, 8, 32768>;
    __shared__ unsigned word[2];
    const int t = threadIdx.x;
    const unsigned G = gridDim.x;
    Claimer<SHARDS, INTERLEAVE> cl{counters, split, nrows, blockIdx.x % SHARDS, 0};
    unsigned row = blockIdx.x, nrow = row + G;
    const bool first_walked = split > 0, second_walked = first_walked && row + G < split;
    if (!second_walked) {
        if (t == 0) {
            const unsigned r0 = first_walked ? row : cl.claim_now();
            word[0] = r0;
            word[1] = r0 < nrows ? cl.claim_now() : nrows;
        }
        __syncthreads();
        row = word[0];
        nrow = word[1];
        __syncthreads();
    }
    if (row >= nrows) return;
    typename M::V cur[M::NL], nxt[M::NL];
    M::load(cur, in, row, t);
    for (unsigned p = 0;; p ^= 1) {
        const bool more = nrow < nrows;               // workgroup-uniform
        const bool walked = nrow + G < split;         // workgroup-uniform
        const bool claims = more && !walked && t == 0;
        unsigned ticket = 0;
        if (claims) ticket = cl.fetch();              // in front of the prefetch
        if (more) M::load(nxt, in, nrow, t);
        M::store(cur, out, row, t);
        if (!more) break;
        if (claims) word[p] = cl.visited >= SHARDS ? nrows : cl.row_of(ticket);
        __syncthreads();
        unsigned claimed = walked ? nrow + G : word[p];
        if (SHARDS > 1 && claimed == ~0u) {           // workgroup-uniform: the shard is empty, walk on to the neighbours
            if (t == 0) word[p ^ 1] = cl.walk_on();
            __syncthreads();
            claimed = word[p ^ 1];
            __syncthreads();
        }
        if (SHARDS == 1 && claimed == ~0u) claimed = nrows;
#pragma unroll
        for (int u = 0; u < M::NL; ++u) cur[u] = nxt[u];
        row = nrow;
        nrow = claimed;
    }
}

__global__ void fill_pattern(unsigned *p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (unsigned)i * 2654435761u + 1u;
}
__global__ void count_wrong(const unsigned *p, size_t n, unsigned long long *wrong)
{
    unsigned long long w = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w += p[i] != (unsigned)i * 2654435761u + 1u;
    if (w) atomicAdd(wrong, w);
}

int main(int argc, char **argv)
{
    const int ROUNDS = argc > 1 ? atoi(argv[1]) : 9, REPS = argc > 2 ? atoi(argv[2]) : 7;
    const size_t bytes = (size_t)2 << 30;
    const unsigned rows32 = (unsigned)(bytes / 32768), rows64 = (unsigned)(bytes / 65536);
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const unsigned G = 2 * (unsigned)prop.multiProcessorCount;
    printf("device %s, %d CUs, grid %u (pair64: %u), %d rounds x %d launches per cell\n", prop.name, prop.multiProcessorCount, G, G / 2, ROUNDS, REPS);
    char *a, *b;
    unsigned *counters;
    unsigned long long *wrong;
    CK(hipMalloc(&a, bytes));
    CK(hipMalloc(&b, bytes));
    CK(hipMalloc(&counters, kCounterBytes));
    CK(hipMalloc(&wrong, 8));
    hipLaunchKernelGGL(fill_pattern, dim3(4096), dim3(256), 0, 0, (unsigned *)a, bytes / 4);
    CK(hipMemset(b, 0, bytes));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    struct Cell { std::string name; std::function<void(const char *, char *)> f; bool claims; std::vector<float> oop, inp; };
    std::vector<Cell> cs;
    const dim3 g1(G), g2(G / 2);
    cs.push_back({"base", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<256, 2, 8, 32768, MAP_BASE>), g1, dim3(256), 0, 0, i, o, rows32); }, false, {}, {}});
    cs.push_back({"rot8", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<256, 2, 8, 32768, MAP_ROT8>), g1, dim3(256), 0, 0, i, o, rows32); }, false, {}, {}});
    cs.push_back({"xcd8th", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<256, 2, 8, 32768, MAP_XCD8TH>), g1, dim3(256), 0, 0, i, o, rows32); }, false, {}, {}});
    cs.push_back({"pair64", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<512, 2, 8, 65536, MAP_BASE>), g2, dim3(512), 0, 0, i, o, rows64); }, false, {}, {}});
    cs.push_back({"pair64w", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<512, 2, 16, 65536, MAP_BASE>), g2, dim3(512), 0, 0, i, o, rows64); }, false, {}, {}});
    cs.push_back({"c64shape", [=](const char *i, char *o) { hipLaunchKernelGGL((copy_walk<256, 2, 16, 65536, MAP_BASE>), g1, dim3(256), 0, 0, i, o, rows64); }, false, {}, {}});
    for (unsigned pct : {25u, 50u, 75u, 100u}) {
        const unsigned split = (rows32 - rows32 / 100 * pct - rows32 % 100 * pct / 100) / G * G;
        cs.push_back({"claim1@" + std::to_string(pct), [=](const char *i, char *o) { hipLaunchKernelGGL((copy_claim<1, false>), g1, dim3(256), 0, 0, i, o, rows32, split, counters); }, true, {}, {}});
        cs.push_back({"claim8@" + std::to_string(pct), [=](const char *i, char *o) { hipLaunchKernelGGL((copy_claim<8, false>), g1, dim3(256), 0, 0, i, o, rows32, split, counters); }, true, {}, {}});
        cs.push_back({"claim8i@" + std::to_string(pct), [=](const char *i, char *o) { hipLaunchKernelGGL((copy_claim<8, true>), g1, dim3(256), 0, 0, i, o, rows32, split, counters); }, true, {}, {}});
        if (pct == 100) cs.push_back({"claim32@" + std::to_string(pct), [=](const char *i, char *o) { hipLaunchKernelGGL((copy_claim<32, false>), g1, dim3(256), 0, 0, i, o, rows32, split, counters); }, true, {}, {}});
    }
    auto run = [&](Cell &c, const char *i, char *o) {
        if (c.claims) (void)hipMemsetAsync(counters, 0, kCounterBytes, 0);
        c.f(i, o);
    };
    // every cell once out of place into a zeroed buffer: all rows copied, each to its own place
    for (auto &c : cs) {
        CK(hipMemset(b, 0, bytes));
        CK(hipMemset(wrong, 0, 8));
        run(c, a, b);
        hipLaunchKernelGGL(count_wrong, dim3(4096), dim3(256), 0, 0, (const unsigned *)b, bytes / 4, wrong);
        unsigned long long w = 0;
        CK(hipMemcpy(&w, wrong, 8, hipMemcpyDeviceToHost));
        CK(hipGetLastError());
        printf("check %-10s %s (%llu words wrong)\n", c.name.c_str(), w ? "WRONG" : "ok", w);
        if (w) return 1;
    }
    for (int r = 0; r < 200; ++r) cs[0].f(a, b);  // clock ramp
    CK(hipDeviceSynchronize());
    for (int r = 0; r < ROUNDS + 1; ++r)  // (round 0 is a warm-up)
        for (auto &c : cs)
            for (int form = 0; form < 2; ++form) {
                std::vector<float> ms;
                for (int k = 0; k < REPS; ++k) {
                    if (c.claims) (void)hipMemsetAsync(counters, 0, kCounterBytes, 0);
                    hipEventRecord(e0);
                    c.f(form ? b : a, b);
                    hipEventRecord(e1);
                    CK(hipEventSynchronize(e1));
                    float t;
                    hipEventElapsedTime(&t, e0, e1);
                    ms.push_back(t);
                }
                std::sort(ms.begin(), ms.end());
                if (r) (form ? c.inp : c.oop).push_back(ms[ms.size() / 2]);
            }
    CK(hipGetLastError());
    float spread = 0;
    printf("%-12s %-8s  median ms   min ms   max ms   of 8 TB/s (median)   vs base\n", "cell", "form");
    for (int form = 0; form < 2; ++form) {
        float base_med = 0;
        for (auto &c : cs) {
            std::vector<float> v = form ? c.inp : c.oop;
            std::sort(v.begin(), v.end());
            const float med = v[v.size() / 2];
            if (&c == &cs[0]) base_med = med;
            spread = std::max(spread, v.back() - v.front());
            printf("%-12s %-8s  %.4f     %.4f   %.4f   %.3f                %+.2f %%\n", c.name.c_str(), form ? "inplace" : "oop", med, v.front(), v.back(),
                   2.0 * bytes / med / 1e6 / 8000.0, 100.0 * (med / base_med - 1.0));
        }
    }
    printf("box spread (largest max - min of one cell's round medians): %.4f ms\n", spread);
    return 0;
}
