"""kofft::cepstrum's mel functions (cepstrum.rs:36-98): triangular mel filterbank energies and MFCCs of f32 magnitude rows on the
device.  The filter edges are an input of the library; everything after them -- the weighted sums, the libm crate's logf, dct::dct2 --
is the reference's arithmetic bit for bit.

``mel_bins`` computes the reference-shaped edges on the host with glibc's log10f / powf (pinned wherever the exact edge is not within
an ulp of an integer; the last edge of an odd n_fft is not: include/kofft_hip.h).  ``mel_filterbank`` and ``mfcc`` take one 1-D row (or
a list of rows) and return new float32 arrays; ``mfcc_batch`` takes a list of 1-D rows of any lengths, one device call per length.
Each accepts ``bins=`` (num_filters + 2 nondecreasing integers) to override the helper's edges -- for instance edges laid over the
win_len / 2 bins of a one-sided spectrum, which the reference cannot express -- and ``fft=``, the f32 HipFftImpl to run on; without
one, a context on device 0 is created at the first call and kept.  Errors are raised before any device is touched: num_coeffs >
num_mel raises FftError(InvalidValue) (cepstrum.rs:79), more than 4096 filters DeviceError.

``mel_from_audio`` and ``mfcc_from_audio`` run the whole front end -- stft_magnitudes, the filterbank, the log and the DCT -- on rows of
samples in one call, with the results of ``stft_magnitudes_rows`` followed by ``mel_filterbank`` / ``mfcc`` bit for bit and without the
magnitudes ever leaving the device; their default edges are ``mel_bins(sample_rate, win_len // 2, num_filters)``.  The ``*_dev`` forms
take device addresses and run asynchronously on the context's stream."""
from __future__ import annotations

from typing import Optional

from .api import HipFftImpl, _direct_ctx, frontend_rows, mel_bins, mel_filterbank_rows, mfcc_rows

__all__ = ["mel_bins", "mel_filterbank", "mfcc", "mfcc_batch", "mel_from_audio", "mfcc_from_audio", "mel_from_audio_dev",
           "mfcc_from_audio_dev"]


def mel_filterbank(fft_mags, sample_rate: float, num_filters: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mel_filterbank (cepstrum.rs:36-69)."""
    return mel_filterbank_rows(fft_mags, sample_rate, num_filters, bins, fft)


def mfcc(fft_mags, sample_rate: float, num_mel: int, num_coeffs: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mfcc (cepstrum.rs:72-85)."""
    return mfcc_rows(fft_mags, sample_rate, num_mel, num_coeffs, bins, fft)


def mfcc_batch(batch, sample_rate: float, num_mel: int, num_coeffs: int, bins=None, fft: Optional[HipFftImpl] = None):
    """cepstrum::mfcc_batch (cepstrum.rs:88-98): a list of 1-D rows in, a list of num_coeffs-long rows out."""
    return mfcc_rows(list(batch), sample_rate, num_mel, num_coeffs, bins, fft)


def mel_from_audio(signals, sample_rate: float, win_len: int, hop: int, num_filters: int, window=None, bins=None,
                   frames: Optional[int] = None, fft: Optional[HipFftImpl] = None):
    """Mel energies of every frame of a 1-D signal ([frames, num_filters] out) or of every row of a 2-D [rows, len] array
    ([rows, frames, num_filters] out).  ``window`` None is hann(win_len); ``frames`` defaults to ceil(len / hop)."""
    return frontend_rows(signals, sample_rate, win_len, hop, num_filters, None, window, bins, frames, fft)


def mfcc_from_audio(signals, sample_rate: float, win_len: int, hop: int, num_mel: int, num_coeffs: int, window=None, bins=None,
                    frames: Optional[int] = None, fft: Optional[HipFftImpl] = None):
    """MFCCs of every frame: [frames, num_coeffs] or [rows, frames, num_coeffs] float32 (see mel_from_audio)."""
    return frontend_rows(signals, sample_rate, win_len, hop, num_mel, int(num_coeffs), window, bins, frames, fft)


def mel_from_audio_dev(d_signal: int, rows: int, length: int, row_stride: int, d_window: int, win_len: int, hop: int, frames: int, bins,
                       d_energies: int, fft: Optional[HipFftImpl] = None) -> None:
    """mel_from_audio on device memory (HipFftImpl.stft_mel_rows_dev): d_window 0 for hann(win_len), `bins` a host array."""
    _direct_ctx(fft).stft_mel_rows_dev(d_signal, rows, length, row_stride, d_window, win_len, hop, frames, bins, d_energies)


def mfcc_from_audio_dev(d_signal: int, rows: int, length: int, row_stride: int, d_window: int, win_len: int, hop: int, frames: int, bins,
                        num_coeffs: int, d_coeffs: int, fft: Optional[HipFftImpl] = None) -> None:
    """mfcc_from_audio on device memory (HipFftImpl.stft_mfcc_rows_dev)."""
    _direct_ctx(fft).stft_mfcc_rows_dev(d_signal, rows, length, row_stride, d_window, win_len, hop, frames, bins, num_coeffs, d_coeffs)
