// tables.h -- host-side planner recipes (see tables.cpp).
#pragma once
#include <stddef.h>
namespace kofft_tables {
void twiddles_f32(size_t n, float *out);   // n/2 complex
void twiddles_f64(size_t n, double *out);
void rfft_table_f32(size_t m, float *out); // m complex
void rfft_table_f64(size_t m, double *out);
void hann_f32(size_t len, float *out);
// DctPlanner (dct.rs:50-58, 89-92): n (cos, sin) pairs of a_k = (PI * k) / (2 * n), all in f32
void dct2_table_f32(size_t n, float *cs);
// dct::dct1..dct4 (dct.rs:108-176) and dst::dst1..dst4 (dst.rs:89-146): the n x n table C[i][k] (row-major, row stride ldc >= n)
// of the direct sums, each entry glibc cosf / sinf of the reference's angle; rows outside the kind's i range are zero, so are
// columns n .. ldc-1.  family 0 = DCT, 1 = DST; type 1..4.  Built on up to 16 host threads.
void direct_range(int family, int type, size_t n, size_t *i_begin, size_t *i_end);
void direct_table_f32(int family, int type, size_t n, size_t ldc, float *c);
// DstPlanner::build_table_offset (dst.rs:41-50): sin(factor * (i + off)), factor = pi_T / T::from_f32(n as f32); off 0.5 (type 2,
// 4) or 0.0 (type 3)
void dst_planner_f32(int type, size_t n, float *out);
void dst_planner_f64(int type, size_t n, double *out);
void bluestein_f32(size_t n, size_t m, float *chirp /* n complex */, float *b /* m complex */);
void bluestein_f64(size_t n, size_t m, double *chirp, double *b);
// fft_radix4 (fft.rs:1455-1548), n a power of four: perm = n source indices, w = radix4_triples(n) x (w1, w2, w3) complex
size_t radix4_triples(size_t n);
void radix4_f32(size_t n, unsigned *perm, float *w);
void radix4_f64(size_t n, unsigned *perm, double *w);
}  // namespace kofft_tables
