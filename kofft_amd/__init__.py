"""kofft_amd -- MI355X (gfx950) implementation of kofft's FFT -> rFFT -> STFT hot path.

The product is ``kofft_amd/lib/libkofft_hip.so`` (hand-written HIP kernels behind the C ABI of
``include/kofft_hip.h``); this package is the Python host mirror of the reference's operator
interface on top of it.  There is no CPU fallback: without the library every call raises.
"""
from .api import (DctPlanner, DeviceError, fft2d_inplace, fft3d_inplace, flatten_2d, flatten_3d, FftError, FftPlan, FftPlanner, FftStrategy, HipFftImpl, HipMulti, IstftStream, RfftPlanner, StftStream, batch,
                  batch_inverse, frame, hann, hilbert_analytic, inverse_frame, inverse_parallel, irfft_packed, istft, istft_onesided, multi_channel, multi_channel_inverse, new_fft_impl, parallel, real_cepstrum, rfft_packed, stft, stft_magnitudes, stft_magnitudes_rows, stft_multi, stft_onesided, stft_rows,
                  ComplexVec, SplitComplex, fft_complex_vec, fft_split, fft_split_complex, ifft_complex_vec, ifft_split, ifft_split_complex)
from ._lib import LibraryMissing, load as load_library
from . import dct, dst  # noqa: E402  (kofft::dct / kofft::dst: the direct transforms, DstPlanner)
from . import wavelet  # noqa: E402  (kofft::wavelet: haar, db2, db4, sym4, coif1)
from . import czt, goertzel  # noqa: E402  (kofft::czt::czt_f32, kofft::goertzel::goertzel_f32)
from . import hartley, window  # noqa: E402  (kofft::hartley::dht, kofft::window / window_more beyond hann)
from . import mfcc  # noqa: E402  (kofft::cepstrum::mel_filterbank / mfcc / mfcc_batch)
from . import spectrogram  # noqa: E402  (kofft::visual::spectrogram: magnitude_to_db, db_scale, the colour maps, log_scale_bins)
from . import convolve  # noqa: E402  (overlap-save FFT convolution / correlation of rows: convolve, correlate, convolve_bank, correlate_bank, default_block)
from . import psd  # noqa: E402  (Welch power spectra and cross spectra of rows: welch, csd, segments)
from . import resample  # noqa: E402  (polyphase resampling of rows: upfirdn, resample_poly, design_taps)
from . import iir  # noqa: E402  (IIR filtering of rows by a cascade of biquads: sosfilt, sosfilt_zi, sosfiltfilt)
from . import mdct  # noqa: E402  (MDCT / IMDCT of rows on a fast DCT-IV: mdct, imdct, dct4, sine_window, vorbis_window, kbd_window)
from . import pfb  # noqa: E402  (polyphase filter bank of rows: analysis, synthesis, prototype, reconstruction)

__all__ = ["DctPlanner", "DeviceError", "fft2d_inplace", "fft3d_inplace", "flatten_2d", "flatten_3d", "FftError", "FftPlan", "FftPlanner", "FftStrategy", "HipFftImpl", "HipMulti", "IstftStream", "RfftPlanner", "StftStream",
           "batch", "batch_inverse", "frame", "hann", "hilbert_analytic", "inverse_frame", "inverse_parallel", "irfft_packed", "istft", "istft_onesided", "multi_channel", "multi_channel_inverse", "new_fft_impl",
           "parallel", "real_cepstrum", "rfft_packed", "stft", "stft_magnitudes", "stft_magnitudes_rows", "stft_multi", "stft_onesided", "stft_rows", "LibraryMissing", "load_library", "dct", "dst", "wavelet", "czt", "goertzel", "hartley", "window", "mfcc", "spectrogram", "convolve", "psd", "resample", "iir", "mdct", "pfb",
           "ComplexVec", "SplitComplex", "fft_complex_vec", "fft_split", "fft_split_complex", "ifft_complex_vec", "ifft_split", "ifft_split_complex"]
__version__ = "0.1.0"
