// hartley_impl.hip.h -- hartley::dht (hartley.rs:12-27) on device pointers, f32 only like the reference.
//
// out[b][k] = sum_i x[b][i] * H[i][k], the sum seeded with +0 and taken in increasing i, one f32 multiply and one f32 add per term
// (never fused): launch_direct<DIR_ZERO> of direct_impl.hip.h (through direct_zero_sums, k_direct_f32.hip), the route rule and the
// kernels of the direct DCT / DST unchanged.  What is new is the table: H[i][k] = cosf(a) + sinf(a), a = factor * ((i * k) as f32),
// factor = (2.0 * PI) / n as f32, with the libm crate's cosf / sinf (libm_trigf.hip.h: f64 polynomials after an f64 reduction), not
// glibc's.  H is symmetric and depends on n only: one table per (context, n) in the context's table cache (kind kTableDht), n rows
// of direct_ldc(n) floats, the padding columns +0.
//  * dht_table_kernel builds it on the device, asynchronously on the context's stream and with no host buffer: a lane owns four
//    consecutive columns of one row and writes them with one 16-byte store, so a wavefront writes 1024 consecutive bytes; a
//    workgroup covers up to 1024 columns of one row.  Per entry about 40 f64 multiplies and adds: at n = 4096 0.7 G of them
//    against 64 MiB of stores.
//  * kofft_hip_set_dht_table_device(ctx, 0): kofft_tables::dht_table_f32 (tables.cpp, the same header compiled for the host, up to
//    16 threads) and a synchronous upload instead -- the same bytes (A/B, tests).
// Measured (tools/bench_hartley.py): the first call of a fresh context on 64 rows takes 0.08 / 0.26 / 1.24 ms at
// n = 256 / 1024 / 4096 with the device-built table, 0.48 / 1.36 / 28.2 ms with the host-built one: the device build is the default.
#pragma once

#include "direct_impl.hip.h"
#include "libm_trigf.hip.h"

namespace kofft {
namespace host {

constexpr int DHT_BLOCK = 256;  // lanes of a workgroup: four columns each, 1024 columns of one row

// grid: (ceil(ldc / (4 * DHT_BLOCK)), n), blockIdx.y = the row i (uniform: its address and i * k need no per-lane multiply-add).
// i * k <= 4095^2 < 2^24: exact in int and in f32.
__global__ __launch_bounds__(DHT_BLOCK) void dht_table_kernel(float *__restrict__ h, const int n, const int ldc, const float factor)
{
    const int k0 = (int)(blockIdx.x * DHT_BLOCK + threadIdx.x) * 4;
    const int i = (int)blockIdx.y;
    if (k0 >= ldc) return;  // (ldc is a multiple of DT_BN = 128 floats: a lane's four columns are all inside or all outside)
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        float v = 0.0f;  // the padding columns
        if (k < n) {
            const float angle = factor * (float)(i * k);  // hartley.rs:19
            v = libm_cosf(angle) + libm_sinf(angle);      // hartley.rs:20-22: re + im
        }
        e[j] = v;
    }
    // 16-byte aligned: the base comes from hipMalloc, ldc is a multiple of DT_BN floats and k0 one of four
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u bits = __builtin_bit_cast(v4u, dt_f4{e[0], e[1], e[2], e[3]});
    *reinterpret_cast<v4u *>(h + (size_t)i * ldc + k0) = bits;
    b128_store_guard(bits);
}

}  // namespace host
}  // namespace kofft
