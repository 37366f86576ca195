// ubench_copy5.hip -- the claim2@87 cell of ubench_copy4.hip (persistent, 32 KiB step, next step prefetched, nt both ways, the last 87 % of
// the rows claimed from two words) launched BACK TO BACK on one stream, varying the direction a launch walks the batch in and the cache
// policy of the rows it touches last and first.  Development tool (round 9): decides whether the 256 MiB Infinity Cache can hand the end
// of one launch to the start of the next one when the 4096-point c32 kernel is called twice on one buffer.
//
// A launch hands out WALK indices w exactly as copy4's copy_claim hands out rows; the memory row is w, or nrows - 1 - w when the launch
// is mirrored.  Rows with w >= keep_from are stored with the default policy instead of nt; rows with w < plain_to are loaded with it.
//
//   cell        direction of launch k      stores of the last T MiB in walk order      loads of the first T MiB in walk order
//   asc         ascending                  nt                                          nt                        (the kernel today)
//   snake@T     k odd: mirrored            default                                     nt        (snake@0: the direction alone)
//   snakep@T    k odd: mirrored            default                                     default
//   keep@T      ascending                  default                                     nt        (what an isolated call pays for the kept tail)
//
//   form        launch k reads / writes
//   inplace     B / B
//   twin        A / B                      (the benchmark's out-of-place twin: same source, same destination)
//   pingpong    k even: A / B, k odd: B / A
//
// Cells are interleaved in one process over ROUNDS rounds; one sample is the mean launch time of REPS launches between two events, behind
// two untimed launches of the same cell (so that the first timed launch follows one of its own kind).  Per cell: median, minimum and
// maximum of its round samples; the box's spread = the largest (max - min) of any one cell.  Every cell is checked once, in both
// directions, out of place against the input.  No launch resets a claim word: every launch of a burst has claim words of its own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
typedef float f2v __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int BLOCK = 256, STEPB = 32768, NL = STEPB / (BLOCK * 8);
constexpr unsigned SHARDS = 2, kLine = 32;  // unsigned per 128-byte line
constexpr size_t kCounterBytes = SHARDS * 128;

struct Walk {
    unsigned nrows, split, mirror, keep_from, plain_to;
};

template <bool NT>
__device__ __forceinline__ void load_row(f2v *r, const char *in, unsigned row, int t)
{
    const f2v *p = reinterpret_cast<const f2v *>(in + (size_t)row * STEPB);
#pragma unroll
    for (int u = 0; u < NL; ++u) r[u] = NT ? __builtin_nontemporal_load(p + t + BLOCK * u) : p[t + BLOCK * u];
}
template <bool NT>
__device__ __forceinline__ void store_row(const f2v *r, char *out, unsigned row, int t)
{
    f2v *p = reinterpret_cast<f2v *>(out + (size_t)row * STEPB);
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        if (NT) __builtin_nontemporal_store(r[u], p + t + BLOCK * u);
        else p[t + BLOCK * u] = r[u];
    }
}

struct Claimer {
    unsigned *counters;
    unsigned split, nrows, shard, visited;
    __device__ __forceinline__ unsigned lo(unsigned s) const { return split + (nrows - split) / SHARDS * s; }
    __device__ __forceinline__ unsigned hi(unsigned s) const { return s + 1 == SHARDS ? nrows : lo(s + 1); }
    __device__ __forceinline__ unsigned row_of(unsigned ticket) const  // a walk index, or ~0u when this shard is exhausted
    {
        const unsigned long long r = (unsigned long long)lo(shard) + ticket;
        return r < hi(shard) ? (unsigned)r : ~0u;
    }
    __device__ __forceinline__ unsigned fetch() { return atomicAdd(counters + shard * kLine, 1u); }
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

// (no __restrict__: the in-place form passes one buffer twice)
__global__ __launch_bounds__(BLOCK, 2) void copy_snake(const char *in, char *out, const Walk wk, unsigned *counters)
{
    __shared__ unsigned word[2];
    const int t = threadIdx.x;
    const unsigned G = gridDim.x, nrows = wk.nrows, split = wk.split;
    Claimer cl{counters, split, nrows, blockIdx.x % SHARDS, 0};
    // every w below is < nrows where it is used as a row: the memory row nrows - 1 - w is in [0, nrows) too
    auto mem = [&](unsigned w) { return wk.mirror ? nrows - 1 - w : w; };
    auto load = [&](f2v *r, unsigned w) {  // workgroup-uniform branch
        if (w < wk.plain_to) load_row<false>(r, in, mem(w), t);
        else load_row<true>(r, in, mem(w), t);
    };
    auto store = [&](const f2v *r, unsigned w) {  // workgroup-uniform branch
        if (w >= wk.keep_from) store_row<false>(r, out, mem(w), t);
        else store_row<true>(r, out, mem(w), t);
    };
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
    f2v cur[NL], nxt[NL];
    load(cur, row);
    for (unsigned p = 0;; p ^= 1) {
        const bool more = nrow < nrows;        // workgroup-uniform
        const bool walked = nrow + G < split;  // workgroup-uniform
        const bool claims = more && !walked && t == 0;
        unsigned ticket = 0;
        if (claims) ticket = cl.fetch();  // in front of the prefetch
        if (more) load(nxt, nrow);
        store(cur, row);
        if (!more) break;
        if (claims) word[p] = cl.visited >= SHARDS ? nrows : cl.row_of(ticket);
        __syncthreads();
        unsigned claimed = walked ? nrow + G : word[p];
        if (claimed == ~0u) {  // workgroup-uniform: the shard is empty, walk on to the neighbours
            if (t == 0) word[p ^ 1] = cl.walk_on();
            __syncthreads();
            claimed = word[p ^ 1];
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) cur[u] = nxt[u];
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
    const int ROUNDS = argc > 1 ? atoi(argv[1]) : 9, REPS = argc > 2 ? atoi(argv[2]) : 16, LEAD = 2;
    const size_t bytes = (size_t)2 << 30;
    const unsigned nrows = (unsigned)(bytes / STEPB), rows_per_mib = (1u << 20) / STEPB;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const unsigned G = 2 * (unsigned)prop.multiProcessorCount;
    const unsigned pct = 87, split = (nrows - nrows / 100 * pct - nrows % 100 * pct / 100) / G * G;
    printf("device %s, %d CUs, grid %u, %u rows, split %u, %d rounds x (%d + %d) launches per cell and form\n", prop.name, prop.multiProcessorCount, G,
           nrows, split, ROUNDS, LEAD, REPS);
    char *a, *b;
    unsigned *counters;
    unsigned long long *wrong;
    const int nsets = LEAD + REPS;
    CK(hipMalloc(&a, bytes));
    CK(hipMalloc(&b, bytes));
    CK(hipMalloc(&counters, kCounterBytes * nsets));
    CK(hipMalloc(&wrong, 8));
    hipLaunchKernelGGL(fill_pattern, dim3(4096), dim3(256), 0, 0, (unsigned *)a, bytes / 4);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    struct Cell { std::string name; bool snake; unsigned keep_mib, plain_mib; std::vector<float> ms[3]; };
    std::vector<Cell> cs;
    cs.push_back({"asc", false, 0, 0, {}});
    for (unsigned T : {0u, 32u, 64u, 128u, 192u, 256u, 384u}) cs.push_back({"snake@" + std::to_string(T), true, T, 0, {}});
    for (unsigned T : {32u, 64u, 128u, 192u, 256u, 384u}) cs.push_back({"snakep@" + std::to_string(T), true, T, T, {}});
    for (unsigned T : {32u, 64u, 128u, 192u, 256u, 384u}) cs.push_back({"keep@" + std::to_string(T), false, T, 0, {}});
    // launch k of a burst: claim words of its own (zeroed in front of the burst)
    auto launch = [&](const Cell &c, int k, const char *i, char *o) {
        const Walk wk{nrows, split, c.snake ? (unsigned)(k & 1) : 0u, nrows - c.keep_mib * rows_per_mib, c.plain_mib * rows_per_mib};
        hipLaunchKernelGGL(copy_snake, dim3(G), dim3(BLOCK), 0, 0, i, o, wk, counters + (size_t)k * SHARDS * kLine);
    };
    const char *forms[3] = {"inplace", "twin", "pingpong"};
    auto burst_launch = [&](const Cell &c, int form, int k) {
        if (form == 0) launch(c, k, b, b);
        else if (form == 1) launch(c, k, a, b);
        else launch(c, k, (k & 1) ? b : a, (k & 1) ? a : b);
    };
    // every cell once per direction, out of place into a zeroed buffer: all rows copied, each to its own place
    for (auto &c : cs)
        for (int k = 0; k < 2; ++k) {
            CK(hipMemset(b, 0, bytes));
            CK(hipMemset(wrong, 0, 8));
            CK(hipMemset(counters, 0, kCounterBytes * nsets));
            launch(c, k, a, b);
            hipLaunchKernelGGL(count_wrong, dim3(4096), dim3(256), 0, 0, (const unsigned *)b, bytes / 4, wrong);
            unsigned long long w = 0;
            CK(hipMemcpy(&w, wrong, 8, hipMemcpyDeviceToHost));
            CK(hipGetLastError());
            if (w) { printf("check %-10s launch %d WRONG (%llu words)\n", c.name.c_str(), k, w); return 1; }
        }
    printf("check: every cell copies every row to its own place in both directions\n");
    CK(hipMemset(counters, 0, kCounterBytes * nsets));
    for (int r = 0; r < 200; ++r) {  // clock ramp
        if (r % nsets == 0) (void)hipMemsetAsync(counters, 0, kCounterBytes * nsets, 0);
        launch(cs[0], r % nsets, a, b);
    }
    CK(hipDeviceSynchronize());
    for (int r = 0; r < ROUNDS + 1; ++r)  // (round 0 is a warm-up)
        for (auto &c : cs)
            for (int form = 0; form < 3; ++form) {
                CK(hipMemsetAsync(counters, 0, kCounterBytes * nsets, 0));
                for (int k = 0; k < LEAD; ++k) burst_launch(c, form, k);
                (void)hipEventRecord(e0);
                for (int k = LEAD; k < LEAD + REPS; ++k) burst_launch(c, form, k);
                (void)hipEventRecord(e1);
                CK(hipEventSynchronize(e1));
                float t;
                (void)hipEventElapsedTime(&t, e0, e1);
                if (r) c.ms[form].push_back(t / REPS);
            }
    CK(hipGetLastError());
    // the data survived every burst (all forms copy the pattern onto itself)
    CK(hipMemset(wrong, 0, 8));
    hipLaunchKernelGGL(count_wrong, dim3(4096), dim3(256), 0, 0, (const unsigned *)a, bytes / 4, wrong);
    hipLaunchKernelGGL(count_wrong, dim3(4096), dim3(256), 0, 0, (const unsigned *)b, bytes / 4, wrong);
    unsigned long long w = 0;
    CK(hipMemcpy(&w, wrong, 8, hipMemcpyDeviceToHost));
    printf("after the bursts: %llu words wrong in A and B\n", w);
    float spread = 0;
    printf("%-12s %-9s  median ms   min ms   max ms   of 8 TB/s (median)   vs asc\n", "cell", "form");
    for (int form = 0; form < 3; ++form) {
        float base_med = 0;
        for (auto &c : cs) {
            std::vector<float> v = c.ms[form];
            std::sort(v.begin(), v.end());
            const float med = v[v.size() / 2];
            if (&c == &cs[0]) base_med = med;
            spread = std::max(spread, v.back() - v.front());
            printf("%-12s %-9s  %.4f     %.4f   %.4f   %.3f                %+.2f %%\n", c.name.c_str(), forms[form], med, v.front(), v.back(),
                   2.0 * bytes / med / 1e6 / 8000.0, 100.0 * (med / base_med - 1.0));
        }
    }
    printf("box spread (largest max - min of one cell's round samples): %.4f ms\n", spread);
    return w ? 1 : 0;
}
