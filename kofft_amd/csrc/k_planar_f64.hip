// k_planar_f64.hip -- FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on planes of double: every kernel instance of the planar
// layout (planar_impl.hip.h).  One translation unit per element type, like the complex transforms, so that `make -j` builds them side by side.
#include "planar_impl.hip.h"

namespace kofft {
namespace host {
template int planar_dev<double>(kofft_hip_ctx *, const double *, const double *, double *, double *, size_t, size_t, int);
}  // namespace host
}  // namespace kofft
