// ubench_logf.hip -- the device's kofft::libm_logf (kofft_amd/csrc/libm_logf.hip.h, the libm crate's logf that the cepstrum kernels
// call) against the same header compiled for the host, on EVERY f32 bit pattern: [1e-12f, FLT_MAX] (what the cepstrum reaches:
// logf(mag + 1e-12f) with mag >= 0) is counted apart from the rest (zeros, subnormals, below 1e-12, negatives, infinities, NaNs).
// Both sides are the same source under -ffp-contract=off; what can differ is the code the two compilers make of it: the division
// (the device's correctly rounded expansion against SSE's divss), subnormal handling, a contraction.  A NaN matches any NaN (the sign
// of a default NaN differs between x86 and gfx950).  Prints the mismatch counts and the first few mismatches.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -o tools/ubench_logf tools/ubench_logf.hip
// run:   tools/ubench_logf
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../kofft_amd/csrc/libm_logf.hip.h"

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));                  \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

__global__ void eval(uint32_t first, uint32_t count, float *out)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        out[i] = kofft::libm_logf(__builtin_bit_cast(float, first + i));
}

static bool same(float a, float b)
{
    if (a != a && b != b) return true;
    return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b);
}

int main()
{
    const uint32_t lo = __builtin_bit_cast(uint32_t, 1e-12f), hi = 0x7f7fffffu;  // [1e-12f, FLT_MAX]
    const uint32_t chunk = 1u << 26;
    const unsigned threads = 16;
    float *d = nullptr;
    CHECK(hipMalloc(&d, chunk * sizeof(float)));
    std::vector<float> h(chunk);
    unsigned long long scanned = 0, in_range = 0, bad_range = 0, bad_other = 0;
    int shown = 0;
    for (uint64_t first = 0; first < (1ull << 32); first += chunk) {
        hipLaunchKernelGGL(eval, dim3(4096), dim3(256), 0, 0, (uint32_t)first, chunk, d);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(h.data(), d, chunk * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<unsigned long long> br(threads, 0), bo(threads, 0), ir(threads, 0);
        std::vector<uint32_t> first_bad(threads, 0xffffffffu);
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                for (uint32_t i = t; i < chunk; i += threads) {
                    const uint32_t bits = (uint32_t)first + i;
                    const bool r = bits >= lo && bits <= hi;
                    ir[t] += r;
                    if (!same(h[i], kofft::libm_logf(__builtin_bit_cast(float, bits)))) {
                        (r ? br[t] : bo[t])++;
                        if (first_bad[t] == 0xffffffffu) first_bad[t] = bits;
                    }
                }
            });
        for (auto &p : pool) p.join();
        for (unsigned t = 0; t < threads; ++t) {
            in_range += ir[t];
            bad_range += br[t];
            bad_other += bo[t];
            if (first_bad[t] != 0xffffffffu && shown < 8) {
                const uint32_t bits = first_bad[t];
                const float x = __builtin_bit_cast(float, bits);
                std::printf("mismatch: x = %a (0x%08x): device 0x%08x host 0x%08x\n", x, bits,
                            __builtin_bit_cast(uint32_t, h[bits - (uint32_t)first]), __builtin_bit_cast(uint32_t, kofft::libm_logf(x)));
                ++shown;
            }
        }
        scanned += chunk;
    }
    CHECK(hipFree(d));
    std::printf("values scanned: %llu (every f32 bit pattern)\n", scanned);
    std::printf("[1e-12f, FLT_MAX]: %llu values, %llu mismatches\n", in_range, bad_range);
    std::printf("the rest (zeros, subnormals, below 1e-12f, negatives, infinities, NaNs): %llu values, %llu mismatches\n", scanned - in_range,
                bad_other);
    // a few pinned values: logf(1) = +0, logf(+inf) = +inf, logf(+-0) = -inf, logf(-1) = NaN, logf(e) ~ 1
    const float pins[] = {1.0f, __builtin_inff(), 0.0f, -0.0f, -1.0f, 2.7182817f, 1e-12f, 1e-45f};
    for (float p : pins) std::printf("libm_logf(%a) = %a\n", p, kofft::libm_logf(p));
    return (bad_range || bad_other) ? 2 : 0;
}
