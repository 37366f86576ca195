"""The expected planes of FftImpl::fft_split / ifft_split (fft.rs:1365-1439): fft_split(re, im) is fft(re + i im) and ifft_split is
ifft, bit for bit (the same butterflies, table and order; ifft_split's conj / conj * scale is ifft's), so the oracle's complex transform
is the reference.  The planes are joined and parted in their own precision (complex64 / complex128): no value is rounded."""
import numpy as np


def split_ref(re: np.ndarray, im: np.ndarray, inverse: bool = False):
    """(re_out, im_out) of oracle.fft(re + 1j * im, inverse) over the last axis; both contiguous, the planes' dtype."""
    from oracle import pyoracle

    re, im = np.ascontiguousarray(re), np.ascontiguousarray(im)
    if re.dtype != im.dtype or re.dtype not in (np.float32, np.float64) or re.shape != im.shape:
        raise TypeError("two planes of one shape, float32 or float64")
    z = np.empty(re.shape, np.complex64 if re.dtype == np.float32 else np.complex128)
    z.real, z.imag = re, im
    out = pyoracle.fft(z, inverse)
    return np.ascontiguousarray(out.real), np.ascontiguousarray(out.imag)
