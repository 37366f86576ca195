"""kofft::cepstrum's mel functions (cepstrum.rs:36-98): triangular mel filterbank energies and MFCCs of f32 magnitude rows on the
device.  The filter edges are an input of the library; everything after them -- the weighted sums, the libm crate's logf, dct::dct2 --
is the reference's arithmetic bit for bit.

``mel_bins`` computes the reference-shaped edges on the host with glibc's log10f / powf (pinned wherever the exact edge is not within
an ulp of an integer; the last edge of an odd n_fft is not: include/kofft_hip.h).  ``mel_filterbank`` and ``mfcc`` take one 1-D row (or
a list of rows) and return new float32 arrays; ``mfcc_batch`` takes a list of 1-D rows of any lengths, one device call per length.
Each accepts ``bins=`` (num_filters + 2 nondecreasing integers) to override the helper's edges -- for instance edges laid over the
win_len / 2 bins of a one-sided spectrum, which the reference cannot express -- and ``fft=``, the f32 HipFftImpl to run on; without
one, a context on device 0 is created at the first call and kept.  Errors are raised before any device is touched: num_coeffs >
num_mel raises FftError(InvalidValue) (cepstrum.rs:79), more than 4096 filters DeviceError."""
from __future__ import annotations

from typing import Optional

from .api import HipFftImpl, mel_bins, mel_filterbank_rows, mfcc_rows

__all__ = ["mel_bins", "mel_filterbank", "mfcc", "mfcc_batch"]


def mel_filterbank(fft_mags, sample_rate: float, num_filters: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mel_filterbank (cepstrum.rs:36-69)."""
    return mel_filterbank_rows(fft_mags, sample_rate, num_filters, bins, fft)


def mfcc(fft_mags, sample_rate: float, num_mel: int, num_coeffs: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mfcc (cepstrum.rs:72-85)."""
    return mfcc_rows(fft_mags, sample_rate, num_mel, num_coeffs, bins, fft)


def mfcc_batch(batch, sample_rate: float, num_mel: int, num_coeffs: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mfcc_batch (cepstrum.rs:88-98): a list of 1-D rows in, a list of num_coeffs-long rows out."""
    return mfcc_rows(list(batch), sample_rate, num_mel, num_coeffs, bins, fft)
