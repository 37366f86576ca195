// kaiser_i0.h -- the modified Bessel function I0 of the Kaiser windows that the host-only filter designs share
// (kofft_hip_resample_taps_f32, kofft_hip_pfb_taps_f32): its power series in double, summed until a term no longer changes the sum.
#pragma once

namespace kofft {
namespace host {

inline double bessel_i0(double x)
{
    const double q = (x / 2.0) * (x / 2.0);
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term = term * (q / ((double)k * (double)k));
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

}  // namespace host
}  // namespace kofft
