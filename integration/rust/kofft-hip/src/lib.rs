//! `HipFftImpl<T>`: a drop-in `kofft::fft::FftImpl<T>` backed by the MI355X library (include/kofft_hip.h).
//!
//! Because `RealFftImpl<T>` is a blanket impl over every `FftImpl<T>` (kofft rfft.rs:837) and `stft()`,
//! `StftStream`, `batch()` are generic over `FftImpl` (stft.rs:76, 160; fft.rs:2156), existing callers
//! only change the type they construct.  The added inherent methods (`fft_batch`, `rfft_batch`,
//! `stft_contiguous`) are the contiguous entry points that escape the `Vec<Vec<_>>` layout.
//!
//! SOURCE ONLY: written against kofft 0.1.5's public API; not compiled in the build image (no rustc).
use core::ffi::{c_char, c_int, c_void};
use core::marker::PhantomData;
use kofft::fft::{Complex, Complex32, Complex64, FftError, FftImpl, FftStrategy};
use kofft::num::Float;

#[repr(C)]
pub struct KofftHipCtx {
    _private: [u8; 0],
}

extern "C" {
    fn kofft_hip_create(device: c_int, out: *mut *mut KofftHipCtx) -> c_int;
    fn kofft_hip_destroy(ctx: *mut KofftHipCtx) -> c_int;
    fn kofft_hip_last_error(ctx: *const KofftHipCtx) -> *const c_char;
    fn kofft_hip_fft_c32(ctx: *mut KofftHipCtx, data: *mut f32, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_fft_c64(ctx: *mut KofftHipCtx, data: *mut f64, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_fft_split_c32(ctx: *mut KofftHipCtx, re: *mut f32, im: *mut f32, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_fft_split_c64(ctx: *mut KofftHipCtx, re: *mut f64, im: *mut f64, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_set_split_fused(ctx: *mut KofftHipCtx, on: c_int) -> c_int;
    fn kofft_hip_fft_radix4_c32(ctx: *mut KofftHipCtx, data: *mut f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_fft_radix4_c64(ctx: *mut KofftHipCtx, data: *mut f64, n: usize, batch: usize) -> c_int;
    fn kofft_hip_fft_c32_strided(ctx: *mut KofftHipCtx, data: *mut f32, len: usize, stride: usize, n: usize, inverse: c_int) -> c_int;
    fn kofft_hip_fft_c64_strided(ctx: *mut KofftHipCtx, data: *mut f64, len: usize, stride: usize, n: usize, inverse: c_int) -> c_int;
    fn kofft_hip_rfft_f32(ctx: *mut KofftHipCtx, input: *const f32, out: *mut f32, window: *const f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_stft_f32(ctx: *mut KofftHipCtx, signal: *const f32, len: usize, window: *const f32, win_len: usize,
                          hop: usize, out: *mut f32, frames: usize) -> c_int;
    fn kofft_hip_stft_parallel_f32(ctx: *mut KofftHipCtx, signal: *const f32, len: usize, window: *const f32, win_len: usize,
                                   hop: usize, out: *mut f32, frames: usize) -> c_int;
    fn kofft_hip_irfft_f32(ctx: *mut KofftHipCtx, input: *const f32, out: *mut f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_istft_f32(ctx: *mut KofftHipCtx, frames_data: *mut f32, frames: usize, window: *const f32, win_len: usize,
                           hop: usize, output: *mut f32, out_len: usize, scratch: *mut f32, scratch_len: usize) -> c_int;
    fn kofft_hip_istft_parallel_f32(ctx: *mut KofftHipCtx, frames_data: *const f32, frames: usize, window: *const f32,
                                    win_len: usize, hop: usize, output: *mut f32, out_len: usize) -> c_int;
    fn kofft_hip_stft_rows_f32(ctx: *mut KofftHipCtx, signal: *const f32, rows: usize, len: usize, row_stride: usize, window: *const f32,
                               win_len: usize, hop: usize, out: *mut f32, frames: usize) -> c_int;
    fn kofft_hip_stft_magnitudes_rows_f32(ctx: *mut KofftHipCtx, samples: *const f32, rows: usize, len: usize, row_stride: usize,
                                          win_len: usize, hop: usize, mags: *mut f32, frames: usize, max_mag: *mut f32) -> c_int;
    fn kofft_hip_istft_rows_f32(ctx: *mut KofftHipCtx, frames_data: *mut f32, rows: usize, frames: usize, window: *const f32,
                                win_len: usize, hop: usize, output: *mut f32, out_len: usize, scratch: *mut f32, scratch_len: usize) -> c_int;
    fn kofft_hip_istft_parallel_rows_f32(ctx: *mut KofftHipCtx, frames_data: *const f32, rows: usize, frames: usize, window: *const f32,
                                         win_len: usize, hop: usize, output: *mut f32, out_len: usize) -> c_int;
    fn kofft_hip_stft_magnitudes_f32(ctx: *mut KofftHipCtx, samples: *const f32, len: usize, win_len: usize, hop: usize,
                                     mags: *mut f32, frames: usize, max_mag: *mut f32) -> c_int;
    fn kofft_hip_czt_f32(ctx: *mut KofftHipCtx, input: *const f32, out: *mut f32, n: usize, m: usize, wr: f32, wi: f32, ar: f32, ai: f32,
                         batch: usize) -> c_int;
    fn kofft_hip_goertzel_f32(ctx: *mut KofftHipCtx, input: *const f32, out: *mut f32, n: usize, batch: usize, sample_rate: f32,
                              target_freqs: *const f32, nfreq: usize) -> c_int;
    fn kofft_hip_set_czt_route(ctx: *mut KofftHipCtx, mode: c_int) -> c_int;
    fn kofft_hip_dht_f32(ctx: *mut KofftHipCtx, input: *const f32, out: *mut f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_set_dht_table_device(ctx: *mut KofftHipCtx, on: c_int) -> c_int;
    fn kofft_hip_mel_filterbank_f32(ctx: *mut KofftHipCtx, mags: *const f32, energies: *mut f32, n_fft: usize, rows: usize, bins: *const u64,
                                    num_mel: usize) -> c_int;
    fn kofft_hip_mfcc_f32(ctx: *mut KofftHipCtx, mags: *const f32, coeffs: *mut f32, n_fft: usize, rows: usize, bins: *const u64,
                          num_mel: usize, num_coeffs: usize) -> c_int;
    fn kofft_hip_set_mfcc_fused(ctx: *mut KofftHipCtx, mode: c_int) -> c_int;
    fn kofft_hip_stft_mel_f32(ctx: *mut KofftHipCtx, signal: *const f32, rows: usize, len: usize, row_stride: usize, window: *const f32,
                              win_len: usize, hop: usize, frames: usize, bins: *const u64, num_mel: usize, energies: *mut f32) -> c_int;
    fn kofft_hip_stft_mfcc_f32(ctx: *mut KofftHipCtx, signal: *const f32, rows: usize, len: usize, row_stride: usize, window: *const f32,
                               win_len: usize, hop: usize, frames: usize, bins: *const u64, num_mel: usize, num_coeffs: usize,
                               coeffs: *mut f32) -> c_int;
    fn kofft_hip_set_frontend_fused(ctx: *mut KofftHipCtx, mode: c_int) -> c_int;
    fn kofft_hip_magnitude_to_db_f32(ctx: *mut KofftHipCtx, mags: *const f32, count: usize, max_mag: *const f32, floor_db: f32, out: *mut f32) -> c_int;
    fn kofft_hip_db_scale_f32(ctx: *mut KofftHipCtx, mags: *const f32, count: usize, max_mag: *const f32, dynamic_range: f32, out: *mut f32) -> c_int;
    fn kofft_hip_spectrogram_render_f32(ctx: *mut KofftHipCtx, mags: *const f32, frames: usize, bins: usize, max_mag: *const f32, mode: c_int,
                                        level: f32, cmap: c_int, depth: c_int, scale: c_int, layout: c_int, pix_of_bin: *const u32,
                                        out: *mut core::ffi::c_void) -> c_int;
    fn kofft_hip_set_spectrogram_transpose(ctx: *mut KofftHipCtx, on: c_int) -> c_int;
    fn kofft_hip_stft_picture_f32(ctx: *mut KofftHipCtx, signal: *const f32, rows: usize, len: usize, row_stride: usize, window: *const f32,
                                  win_len: usize, hop: usize, frames: usize, max_mode: c_int, max_in: *const f32, max_out: *mut f32, mode: c_int,
                                  level: f32, cmap: c_int, depth: c_int, channels: c_int, scale: c_int, layout: c_int, pix_of_bin: *const u32,
                                  out: *mut core::ffi::c_void) -> c_int;
    fn kofft_hip_window_f32(kind: c_int, len: usize, param: f32, out: *mut f32) -> c_int;
    fn kofft_hip_fftnd_c32(ctx: *mut KofftHipCtx, data: *mut f32, depth: usize, rows: usize, cols: usize, inverse: c_int) -> c_int;
    fn kofft_hip_fftnd_c64(ctx: *mut KofftHipCtx, data: *mut f64, depth: usize, rows: usize, cols: usize, inverse: c_int) -> c_int;
    // multi-GPU: one process, one context per device, optional RCCL all-gather (include/kofft_hip.h, "multi-GPU")
    fn kofft_hip_multi_create(ngpu: c_int, devices: *const c_int, out: *mut *mut KofftHipMulti) -> c_int;
    fn kofft_hip_multi_destroy(m: *mut KofftHipMulti) -> c_int;
    fn kofft_hip_multi_last_error(m: *const KofftHipMulti) -> *const c_char;
    fn kofft_hip_multi_stft_f32(m: *mut KofftHipMulti, signal: *const f32, len: usize, window: *const f32, win_len: usize,
                                hop: usize, out: *mut f32, frames: usize, allgather: c_int, d_out_per_gpu: *mut *mut f32) -> c_int;
    fn kofft_hip_stft_f32_multi(ngpu: c_int, signal: *const f32, len: usize, window: *const f32, win_len: usize, hop: usize,
                                out: *mut f32, frames: usize, allgather: c_int) -> c_int;
    fn kofft_hip_multi_fft_c32(m: *mut KofftHipMulti, data: *mut f32, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_multi_fft_c64(m: *mut KofftHipMulti, data: *mut f64, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_multi_rfft_f32(m: *mut KofftHipMulti, input: *const f32, out: *mut f32, window: *const f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_multi_shard(m: *const KofftHipMulti, total: usize, rank: c_int, first: *mut usize, count: *mut usize) -> c_int;
    fn kofft_hip_multi_stft_slice(m: *const KofftHipMulti, len: usize, win_len: usize, hop: usize, frames: usize, rank: c_int,
                                  first_sample: *mut usize, count: *mut usize) -> c_int;
    fn kofft_hip_multi_synchronize(m: *mut KofftHipMulti) -> c_int;
    fn kofft_hip_multi_last_timing_ex(m: *const KofftHipMulti, upload_ms: *mut f32, kernel_ms: *mut f32, gather_ms: *mut f32,
                                      download_ms: *mut f32, wall_ms: *mut f32) -> c_int;
    fn kofft_hip_multi_set_gather(m: *mut KofftHipMulti, mode: c_int) -> c_int;
    fn kofft_hip_multi_gather_mode(m: *const KofftHipMulti, configured: *mut c_int, last: *mut c_int) -> c_int;
    // device-resident twins: one device pointer per device, asynchronous
    fn kofft_hip_multi_fft_c32_dev(m: *mut KofftHipMulti, d_data_per_gpu: *const *mut f32, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_multi_fft_c64_dev(m: *mut KofftHipMulti, d_data_per_gpu: *const *mut f64, n: usize, batch: usize, inverse: c_int) -> c_int;
    fn kofft_hip_multi_rfft_f32_dev(m: *mut KofftHipMulti, d_in_per_gpu: *const *const f32, d_out_per_gpu: *const *mut f32,
                                    d_window_per_gpu: *const *const f32, n: usize, batch: usize) -> c_int;
    fn kofft_hip_multi_stft_f32_dev(m: *mut KofftHipMulti, d_signal_per_gpu: *const *const f32, len: usize,
                                    d_window_per_gpu: *const *const f32, win_len: usize, hop: usize, frames: usize, allgather: c_int,
                                    d_out_per_gpu: *mut *mut f32) -> c_int;
}

/// Slowest device's time in each phase of the last multi-GPU call (HIP events), milliseconds; absent phases are 0.
#[derive(Debug, Default, Clone, Copy)]
pub struct MultiTiming {
    pub upload_ms: f32,
    pub kernel_ms: f32,
    pub gather_ms: f32,
    pub download_ms: f32,
    pub wall_ms: f32,
}

#[repr(C)]
pub struct KofftHipMulti {
    _private: [u8; 0],
}

/// 0 = Ok, 1..=6 = FftError in declaration order (kofft fft.rs:447-454).  FftError has no variant for a
/// device failure, so a negative status (HIP error, unsupported length) panics with the library's message.
fn status(ctx: *const KofftHipCtx, rc: c_int) -> Result<(), FftError> {
    match rc {
        0 => Ok(()),
        1 => Err(FftError::EmptyInput),
        2 => Err(FftError::NonPowerOfTwoNoStd),
        3 => Err(FftError::MismatchedLengths),
        4 => Err(FftError::InvalidStride),
        5 => Err(FftError::InvalidHopSize),
        6 => Err(FftError::InvalidValue),
        _ => {
            let msg = unsafe { std::ffi::CStr::from_ptr(kofft_hip_last_error(ctx)) }.to_string_lossy().into_owned();
            panic!("kofft-hip device error {rc}: {msg}");
        }
    }
}

/// One device context per instance; `Send` but not `Sync`, like `ScalarFftImpl` (kofft fft.rs:589-605).
pub struct HipFftImpl<T: Float> {
    ctx: *mut KofftHipCtx,
    /// `fft_with_strategy(.., Radix4)` reproduces kofft's `fft_radix4` bytes (fft.rs:1356, 1455-1548; NOT a DFT from n = 16):
    /// strict drop-in, ON by default.  `KOFFT_HIP_RADIX4_COMPAT=0`, or `false` set by the caller, opts out (the true
    /// transform for every strategy).
    pub radix4_compat: bool,
    _t: PhantomData<T>,
}

unsafe impl<T: Float> Send for HipFftImpl<T> {}

impl<T: Float> HipFftImpl<T> {
    pub fn new(device: i32) -> Self {
        let mut ctx = core::ptr::null_mut();
        let rc = unsafe { kofft_hip_create(device as c_int, &mut ctx) };
        assert!(rc == 0 && !ctx.is_null(), "kofft_hip_create failed: {rc}");
        let radix4_compat = std::env::var("KOFFT_HIP_RADIX4_COMPAT").map_or(true, |v| v != "0");
        Self { ctx, radix4_compat, _t: PhantomData }
    }
}

impl<T: Float> Default for HipFftImpl<T> {
    fn default() -> Self {
        Self::new(0)
    }
}

impl<T: Float> Drop for HipFftImpl<T> {
    fn drop(&mut self) {
        unsafe { kofft_hip_destroy(self.ctx) };
    }
}

macro_rules! impl_fft {
    ($t:ty, $cplx:ty, $fft:ident, $strided:ident, $radix4:ident, $split:ident) => {
        impl FftImpl<$t> for HipFftImpl<$t> {
            // Complex<T> is #[repr(C)] {re, im} (kofft num.rs:105-110, tests/complex_repr.rs): a slice of n
            // complex values is 2n scalars.
            fn fft(&self, input: &mut [$cplx]) -> Result<(), FftError> {
                status(self.ctx, unsafe { $fft(self.ctx, input.as_mut_ptr() as *mut $t, input.len(), 1, 0) })
            }
            fn ifft(&self, input: &mut [$cplx]) -> Result<(), FftError> {
                status(self.ctx, unsafe { $fft(self.ctx, input.as_mut_ptr() as *mut $t, input.len(), 1, 1) })
            }
            fn fft_strided(&self, input: &mut [$cplx], stride: usize, scratch: &mut [$cplx]) -> Result<(), FftError> {
                status(self.ctx, unsafe {
                    $strided(self.ctx, input.as_mut_ptr() as *mut $t, input.len(), stride, scratch.len(), 0)
                })
            }
            fn ifft_strided(&self, input: &mut [$cplx], stride: usize, scratch: &mut [$cplx]) -> Result<(), FftError> {
                status(self.ctx, unsafe {
                    $strided(self.ctx, input.as_mut_ptr() as *mut $t, input.len(), stride, scratch.len(), 1)
                })
            }
            fn fft_out_of_place_strided(&self, input: &[$cplx], in_stride: usize, output: &mut [$cplx],
                                        out_stride: usize) -> Result<(), FftError> {
                // same checks, same order as kofft fft.rs:1268-1277
                if in_stride == 0 || out_stride == 0 { return Err(FftError::InvalidStride); }
                if input.len() % in_stride != 0 || output.len() % out_stride != 0 { return Err(FftError::InvalidStride); }
                let n = input.len() / in_stride;
                if output.len() / out_stride != n { return Err(FftError::MismatchedLengths); }
                let mut scratch: Vec<$cplx> = (0..n).map(|i| input[i * in_stride]).collect();
                self.fft(&mut scratch)?;
                for i in 0..n { output[i * out_stride] = scratch[i]; }
                Ok(())
            }
            fn ifft_out_of_place_strided(&self, input: &[$cplx], in_stride: usize, output: &mut [$cplx],
                                         out_stride: usize) -> Result<(), FftError> {
                if in_stride == 0 || out_stride == 0 { return Err(FftError::InvalidStride); }
                if input.len() % in_stride != 0 || output.len() % out_stride != 0 { return Err(FftError::InvalidStride); }
                let n = input.len() / in_stride;
                if output.len() / out_stride != n { return Err(FftError::MismatchedLengths); }
                let mut scratch: Vec<$cplx> = (0..n).map(|i| input[i * in_stride]).collect();
                self.ifft(&mut scratch)?;
                for i in 0..n { output[i * out_stride] = scratch[i]; }
                Ok(())
            }
            // kofft fft.rs:1365-1439: the SoA entries override the trait's pack / fft / unpack defaults (fft.rs:556-586) -- the
            // planes go to the device as they are (kofft_hip_fft_split_*), the bytes are those of fft / ifft on re + i im.
            fn fft_split(&self, re: &mut [$t], im: &mut [$t]) -> Result<(), FftError> {
                if re.len() != im.len() { return Err(FftError::MismatchedLengths); }
                status(self.ctx, unsafe { $split(self.ctx, re.as_mut_ptr(), im.as_mut_ptr(), re.len(), 1, 0) })
            }
            fn ifft_split(&self, re: &mut [$t], im: &mut [$t]) -> Result<(), FftError> {
                if re.len() != im.len() { return Err(FftError::MismatchedLengths); }
                status(self.ctx, unsafe { $split(self.ctx, re.as_mut_ptr(), im.as_mut_ptr(), re.len(), 1, 1) })
            }
            fn fft_with_strategy(&self, input: &mut [$cplx], strategy: FftStrategy) -> Result<(), FftError> {
                // kofft fft.rs:1337-1363: Radix2 / SplitRadix / Auto run the Stockham path (fft and stockham_fft agree for
                // n >= 2); Radix4 runs the crate's fft_radix4 arm (fft.rs:1356) byte for byte -- not a DFT from n = 16 (its
                // digit-reversal loop is wrong), but a drop-in returns what the crate returns.  `radix4_compat = false`
                // opts out.
                if input.is_empty() { return Err(FftError::EmptyInput); }
                if input.len() == 1 { return Ok(()); }
                if strategy == FftStrategy::Radix4 && self.radix4_compat { return self.fft_radix4(input); }
                self.fft(input)
            }
        }

        impl HipFftImpl<$t> {
            /// `ScalarFftImpl::fft_radix4` (kofft fft.rs:1455-1548), byte for byte.
            pub fn fft_radix4(&self, input: &mut [$cplx]) -> Result<(), FftError> {
                status(self.ctx, unsafe { $radix4(self.ctx, input.as_mut_ptr() as *mut $t, input.len(), 1) })
            }
        }

        impl HipFftImpl<$t> {
            /// `fft_split` / `ifft_split` on every row of two contiguous `[batch * n]` planes, in place (one kernel launch for the
            /// powers of two up to 2^14 / 2^13).
            pub fn fft_split_batch(&self, re: &mut [$t], im: &mut [$t], n: usize, inverse: bool) -> Result<(), FftError> {
                if re.len() != im.len() || (n != 0 && re.len() % n != 0) { return Err(FftError::MismatchedLengths); }
                let batch = if n == 0 { 1 } else { re.len() / n };
                status(self.ctx, unsafe { $split(self.ctx, re.as_mut_ptr(), im.as_mut_ptr(), n, batch, inverse as c_int) })
            }
            /// `false`: every planar transform of this context through pack, n-point transform, unpack (the same bytes; A/B, tests).
            pub fn set_split_fused(&self, on: bool) -> Result<(), FftError> {
                status(self.ctx, unsafe { kofft_hip_set_split_fused(self.ctx, on as c_int) })
            }
            /// `fft::batch` over one contiguous `[batch * n]` buffer (one kernel launch).
            pub fn fft_batch(&self, data: &mut [$cplx], n: usize, inverse: bool) -> Result<(), FftError> {
                if n != 0 && data.len() % n != 0 { return Err(FftError::MismatchedLengths); }
                let batch = if n == 0 { 1 } else { data.len() / n };
                status(self.ctx, unsafe { $fft(self.ctx, data.as_mut_ptr() as *mut $t, n, batch, inverse as c_int) })
            }
        }
    };
}

impl_fft!(f32, Complex32, kofft_hip_fft_c32, kofft_hip_fft_c32_strided, kofft_hip_fft_radix4_c32, kofft_hip_fft_split_c32);
impl_fft!(f64, Complex64, kofft_hip_fft_c64, kofft_hip_fft_c64_strided, kofft_hip_fft_radix4_c64, kofft_hip_fft_split_c64);

macro_rules! impl_ndfft {
    ($t:ty, $cplx:ty, $nd:ident) => {
        impl HipFftImpl<$t> {
            /// `ndfft::fft2d_inplace` (kofft ndfft.rs:74-101): kofft's function takes `&ScalarFftImpl<T>` concretely,
            /// so the device version is an inherent method with the same length checks.
            pub fn fft2d_inplace(&self, data: &mut [$cplx], rows: usize, cols: usize, scratch_col: &mut [$cplx]) -> Result<(), FftError> {
                if rows * cols != data.len() { return Err(FftError::MismatchedLengths); }
                if rows == 0 || cols == 0 { return Ok(()); }
                if scratch_col.len() != rows { return Err(FftError::MismatchedLengths); }
                status(self.ctx, unsafe { $nd(self.ctx, data.as_mut_ptr() as *mut $t, 1, rows, cols, 0) })
            }
            /// `ndfft::fft3d_inplace` (kofft ndfft.rs:114-155).
            pub fn fft3d_inplace(&self, data: &mut [$cplx], depth: usize, rows: usize, cols: usize, tube: &mut [$cplx],
                                 row: &mut [$cplx], col: &mut [$cplx]) -> Result<(), FftError> {
                if depth * rows * cols != data.len() { return Err(FftError::MismatchedLengths); }
                if depth == 0 || rows == 0 || cols == 0 { return Ok(()); }
                if tube.len() != depth || row.len() != rows || col.len() != cols { return Err(FftError::MismatchedLengths); }
                status(self.ctx, unsafe { $nd(self.ctx, data.as_mut_ptr() as *mut $t, depth, rows, cols, 0) })
            }
        }
    };
}
impl_ndfft!(f32, Complex32, kofft_hip_fftnd_c32);
impl_ndfft!(f64, Complex64, kofft_hip_fftnd_c64);

impl HipFftImpl<f32> {
    /// Batched real FFT with an optional fused window: `out` holds `batch * (n/2 + 1)` complex values.
    pub fn rfft_batch(&self, input: &[f32], n: usize, window: Option<&[f32]>, out: &mut [Complex<f32>]) -> Result<(), FftError> {
        if n == 0 { return Err(FftError::EmptyInput); }
        let batch = input.len() / n;
        if input.len() % n != 0 || out.len() != batch * (n / 2 + 1) { return Err(FftError::MismatchedLengths); }
        if let Some(w) = window { if w.len() != n { return Err(FftError::MismatchedLengths); } }
        let wp = window.map_or(core::ptr::null(), |w| w.as_ptr());
        status(self.ctx, unsafe { kofft_hip_rfft_f32(self.ctx, input.as_ptr(), out.as_mut_ptr() as *mut f32, wp, n, batch) })
    }

    /// `stft::stft` into one contiguous `frames * window.len()` buffer (same checks as kofft stft.rs:83-89).
    pub fn stft_contiguous(&self, signal: &[f32], window: &[f32], hop_size: usize, out: &mut [Complex32]) -> Result<(), FftError> {
        let frames = if window.is_empty() { 0 } else { out.len() / window.len() };
        status(self.ctx, unsafe {
            kofft_hip_stft_f32(self.ctx, signal.as_ptr(), signal.len(), window.as_ptr(), window.len(), hop_size,
                               out.as_mut_ptr() as *mut f32, frames)
        })
    }
}

impl HipFftImpl<f32> {
    /// `stft::parallel` (kofft stft.rs:232-263) ignores the `fft` it is handed and builds a `ScalarFftImpl` per
    /// frame; this is the same arithmetic on the device (only `hop_size == 0` is rejected, as there).
    pub fn stft_parallel_contiguous(&self, signal: &[f32], window: &[f32], hop_size: usize, out: &mut [Complex32]) -> Result<(), FftError> {
        let frames = if window.is_empty() { 0 } else { out.len() / window.len() };
        status(self.ctx, unsafe {
            kofft_hip_stft_parallel_f32(self.ctx, signal.as_ptr(), signal.len(), window.as_ptr(), window.len(), hop_size,
                                        out.as_mut_ptr() as *mut f32, frames)
        })
    }

    /// Batched `irfft` (kofft rfft.rs:468-508): `input` holds `batch * (n/2 + 1)` complex values, `out` `batch * n` reals.
    pub fn irfft_batch(&self, input: &[Complex32], n: usize, out: &mut [f32]) -> Result<(), FftError> {
        if n == 0 { return Err(FftError::EmptyInput); }
        let batch = out.len() / n;
        if out.len() % n != 0 || input.len() != batch * (n / 2 + 1) { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe { kofft_hip_irfft_f32(self.ctx, input.as_ptr() as *const f32, out.as_mut_ptr(), n, batch) })
    }

    /// `stft::istft` (kofft stft.rs:117-156) over one contiguous `frames * window.len()` buffer: the frames are
    /// inverse-transformed in place, `output` is accumulated into and normalised, `scratch` receives the window-square sums.
    pub fn istft_contiguous(&self, frames: &mut [Complex32], window: &[f32], hop_size: usize, output: &mut [f32],
                            scratch: &mut [f32]) -> Result<(), FftError> {
        let count = if window.is_empty() { 0 } else { frames.len() / window.len() };
        status(self.ctx, unsafe {
            kofft_hip_istft_f32(self.ctx, frames.as_mut_ptr() as *mut f32, count, window.as_ptr(), window.len(), hop_size,
                                output.as_mut_ptr(), output.len(), scratch.as_mut_ptr(), scratch.len())
        })
    }

    /// `stft::inverse_parallel` (kofft stft.rs:289-343): frames untouched, tiny-norm samples set to zero.
    pub fn inverse_parallel_contiguous(&self, frames: &[Complex32], window: &[f32], hop_size: usize, output: &mut [f32]) -> Result<(), FftError> {
        let count = if window.is_empty() { 0 } else { frames.len() / window.len() };
        status(self.ctx, unsafe {
            kofft_hip_istft_parallel_f32(self.ctx, frames.as_ptr() as *const f32, count, window.as_ptr(), window.len(), hop_size,
                                         output.as_mut_ptr(), output.len())
        })
    }

    /// `stft::stft` of every row of `signals` (`rows` dense rows of `signals.len() / rows` samples) in one call: `out` holds
    /// `rows * frames * window.len()` values, row r what `stft_contiguous` gives for signal r alone.
    pub fn stft_rows(&self, signals: &[f32], rows: usize, window: &[f32], hop_size: usize, out: &mut [Complex32]) -> Result<(), FftError> {
        if hop_size == 0 { return Err(FftError::InvalidHopSize); }
        if rows == 0 { return Ok(()); }
        if signals.len() % rows != 0 { return Err(FftError::MismatchedLengths); }
        let len = signals.len() / rows;
        let frames = if window.is_empty() { 0 } else { out.len() / (rows * window.len()) };
        status(self.ctx, unsafe {
            kofft_hip_stft_rows_f32(self.ctx, signals.as_ptr(), rows, len, len, window.as_ptr(), window.len(), hop_size,
                                    out.as_mut_ptr() as *mut f32, frames)
        })
    }

    /// `visual::spectrogram::stft_magnitudes` (kofft visual/spectrogram.rs:52-76): magnitudes of bins
    /// `0 .. win_len/2` of every Hann-windowed frame (row-major `frames x win_len/2`) and their maximum.
    pub fn stft_magnitudes(&self, samples: &[f32], win_len: usize, hop: usize) -> Result<(Vec<Vec<f32>>, f32), FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        let frames = (samples.len() + hop - 1) / hop;
        let half = win_len / 2;
        let mut flat = vec![0.0f32; frames * half];
        let mut max_mag = 0.0f32;
        status(self.ctx, unsafe {
            kofft_hip_stft_magnitudes_f32(self.ctx, samples.as_ptr(), samples.len(), win_len, hop, flat.as_mut_ptr(), frames, &mut max_mag)
        })?;
        Ok((flat.chunks(half.max(1)).take(frames).map(|c| c.to_vec()).collect(), max_mag))
    }
}

impl HipFftImpl<f32> {
    /// `czt::czt_f32` (kofft czt.rs:16-54) with the reference's signature: `m` bins of the chirp-Z transform of one real signal.
    pub fn czt_f32(&self, input: &[f32], m: usize, w: (f32, f32), a: (f32, f32)) -> Vec<(f32, f32)> {
        let mut out = vec![(0.0f32, 0.0f32); m];
        self.czt_batch(input, input.len(), m, w, a, &mut out).expect("one row within the library's bounds (n, m <= 4096)");
        out
    }

    /// Batched form: `input` holds rows of `n` reals, `out` as many rows of `m` bins.
    pub fn czt_batch(&self, input: &[f32], n: usize, m: usize, w: (f32, f32), a: (f32, f32), out: &mut [(f32, f32)]) -> Result<(), FftError> {
        let batch = if n == 0 { if m == 0 { 0 } else { out.len() / m } } else { input.len() / n };
        if (n != 0 && input.len() % n != 0) || out.len() != batch * m { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe {
            kofft_hip_czt_f32(self.ctx, input.as_ptr(), out.as_mut_ptr() as *mut f32, n, m, w.0, w.1, a.0, a.1, batch)
        })
    }

    /// 0: the route chosen by batch and by whether the table is already there; 1: sums on the fly; 2: a device-built table (the same bytes).
    pub fn set_czt_route(&self, mode: i32) -> Result<(), FftError> {
        status(self.ctx, unsafe { kofft_hip_set_czt_route(self.ctx, mode as c_int) })
    }

    /// `goertzel::goertzel_f32` (kofft goertzel.rs:16-36) with the reference's signature and errors.
    pub fn goertzel_f32(&self, input: &[f32], sample_rate: f32, target_freq: f32) -> Result<f32, FftError> {
        let mut out = [0.0f32];
        self.goertzel_batch(input, input.len(), sample_rate, &[target_freq], &mut out)?;
        Ok(out[0])
    }

    /// Batched form: rows of `n` samples against every one of `target_freqs`; `out` holds `batch * target_freqs.len()` magnitudes.
    pub fn goertzel_batch(&self, input: &[f32], n: usize, sample_rate: f32, target_freqs: &[f32], out: &mut [f32]) -> Result<(), FftError> {
        if n == 0 { return Err(FftError::EmptyInput); }
        let batch = input.len() / n;
        if input.len() % n != 0 || out.len() != batch * target_freqs.len() { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe {
            kofft_hip_goertzel_f32(self.ctx, input.as_ptr(), out.as_mut_ptr(), n, batch, sample_rate, target_freqs.as_ptr(), target_freqs.len())
        })
    }
}

impl HipFftImpl<f32> {
    /// `hartley::dht` (kofft hartley.rs:12-27) of every row of `n` reals in `input`, into `out` (the same length): the reference's
    /// sums bit for bit, the libm crate's cosf / sinf in the table.  `n == 0` is an empty result; `n > 4096` panics (the table bound).
    pub fn dht_batch(&self, input: &[f32], n: usize, out: &mut [f32]) -> Result<(), FftError> {
        if out.len() != input.len() || (n != 0 && input.len() % n != 0) || (n == 0 && !input.is_empty()) { return Err(FftError::MismatchedLengths); }
        if n == 0 { return Ok(()); }
        status(self.ctx, unsafe { kofft_hip_dht_f32(self.ctx, input.as_ptr(), out.as_mut_ptr(), n, input.len() / n) })
    }

    /// `true` (the default): the Hartley table of a new length is built by a kernel; `false`: on the host and uploaded (the same bytes).
    pub fn set_dht_table_device(&self, on: bool) -> Result<(), FftError> {
        status(self.ctx, unsafe { kofft_hip_set_dht_table_device(self.ctx, on as c_int) })
    }
}

impl HipFftImpl<f32> {
    /// `cepstrum::mel_filterbank`'s sums (kofft cepstrum.rs:51-67) on every row of `n_fft` magnitudes in `mags`, with the filter
    /// edges `bins` (`num_mel + 2` nondecreasing values): `out` receives rows of `num_mel` energies, bit for bit.  Edges out of order
    /// are `InvalidValue` (the reference underflows a `usize`); more than 4096 filters or rows over 2^24 panic.
    pub fn mel_filterbank_batch(&self, mags: &[f32], n_fft: usize, bins: &[u64], out: &mut [f32]) -> Result<(), FftError> {
        if bins.len() < 2 || (n_fft != 0 && mags.len() % n_fft != 0) || (n_fft == 0 && !mags.is_empty()) { return Err(FftError::MismatchedLengths); }
        let num_mel = bins.len() - 2;
        let rows = if n_fft != 0 { mags.len() / n_fft } else if num_mel != 0 { out.len() / num_mel } else { 0 };
        if out.len() != rows * num_mel { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe { kofft_hip_mel_filterbank_f32(self.ctx, mags.as_ptr(), out.as_mut_ptr(), n_fft, rows, bins.as_ptr(), num_mel) })
    }

    /// `cepstrum::mfcc` (kofft cepstrum.rs:72-85) on every row: `out` receives rows of `num_coeffs` coefficients.  `num_coeffs >
    /// num_mel` is `InvalidValue`, checked first like the reference (cepstrum.rs:79).
    pub fn mfcc_rows(&self, mags: &[f32], n_fft: usize, bins: &[u64], num_coeffs: usize, out: &mut [f32]) -> Result<(), FftError> {
        if bins.len() >= 2 && num_coeffs > bins.len() - 2 { return Err(FftError::InvalidValue); }
        if bins.len() < 2 || (n_fft != 0 && mags.len() % n_fft != 0) || (n_fft == 0 && !mags.is_empty()) { return Err(FftError::MismatchedLengths); }
        let rows = if n_fft != 0 { mags.len() / n_fft } else if num_coeffs != 0 { out.len() / num_coeffs } else { 0 };
        if out.len() != rows * num_coeffs { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe {
            kofft_hip_mfcc_f32(self.ctx, mags.as_ptr(), out.as_mut_ptr(), n_fft, rows, bins.as_ptr(), bins.len() - 2, num_coeffs)
        })
    }

    /// 1 (the default): the fused kernel where it measured faster; 0: every MFCC composed; 2: fused wherever it fits (the same bytes).
    pub fn set_mfcc_fused(&self, mode: i32) -> Result<(), FftError> {
        status(self.ctx, unsafe { kofft_hip_set_mfcc_fused(self.ctx, mode as c_int) })
    }

    /// The audio front end in one call: `stft_magnitudes` -> `mel_filterbank` (`num_coeffs` `None`) or -> `mfcc` of every row of `len`
    /// samples in `signals`, `frames` frames per row, with the filter edges `bins` over the `win_len / 2` magnitudes of a frame.  `out`
    /// receives rows * frames rows of `num_mel` energies or `num_coeffs` coefficients, bit for bit what the two calls return; the
    /// magnitudes stay on the device.  `window` `None` is `window::hann(win_len)`.
    #[allow(clippy::too_many_arguments)]
    pub fn stft_mel_rows(&self, signals: &[f32], len: usize, window: Option<&[f32]>, win_len: usize, hop: usize, frames: usize, bins: &[u64],
                         num_coeffs: Option<usize>, out: &mut [f32]) -> Result<(), FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        if let Some(nc) = num_coeffs { if bins.len() >= 2 && nc > bins.len() - 2 { return Err(FftError::InvalidValue); } }
        if bins.len() < 2 || (len != 0 && signals.len() % len != 0) || (len == 0 && !signals.is_empty()) { return Err(FftError::MismatchedLengths); }
        if let Some(w) = window { if w.len() != win_len { return Err(FftError::MismatchedLengths); } }
        let num_mel = bins.len() - 2;
        let width = num_coeffs.unwrap_or(num_mel);
        let rows = if len != 0 { signals.len() / len } else if frames * width != 0 { out.len() / (frames * width) } else { 0 };
        if out.len() != rows * frames * width { return Err(FftError::MismatchedLengths); }
        let win = window.map_or(std::ptr::null(), |w| w.as_ptr());
        status(self.ctx, unsafe {
            match num_coeffs {
                None => kofft_hip_stft_mel_f32(self.ctx, signals.as_ptr(), rows, len, len, win, win_len, hop, frames, bins.as_ptr(), num_mel, out.as_mut_ptr()),
                Some(nc) => kofft_hip_stft_mfcc_f32(self.ctx, signals.as_ptr(), rows, len, len, win, win_len, hop, frames, bins.as_ptr(), num_mel, nc,
                                                    out.as_mut_ptr()),
            }
        })
    }

    /// 1 (the default): the measured choice; 0: every front-end call composed; 2: the fused kernel wherever it fits (the same bytes).
    pub fn set_frontend_fused(&self, mode: i32) -> Result<(), FftError> {
        status(self.ctx, unsafe { kofft_hip_set_frontend_fused(self.ctx, mode as c_int) })
    }
}

/// `kofft::cepstrum`'s mel functions (cepstrum.rs:36-98) on the device, the reference's three functions with a context in front.
/// The edges are computed HERE, with the `libm` crate's own `log10f` / `powf` / `floorf` -- the functions the reference calls -- and
/// passed down, so the results are the reference's bit for bit at every setting, the odd `n_fft` whose last edge the library's
/// glibc-based helper (`kofft_hip_mel_bins_f32`) cannot pin included.
pub mod cepstrum {
    use super::HipFftImpl;
    use kofft::fft::FftError;
    use libm::{floorf, log10f, powf};

    /// cepstrum.rs:38-50, verbatim: the `num_filters + 2` filter edges for rows of `n_fft` magnitudes.
    pub fn mel_bins(sample_rate: f32, n_fft: usize, num_filters: usize) -> Vec<u64> {
        let f_min = 0.0;
        let f_max = sample_rate / 2.0;
        let mel_min = 2595.0 * log10f(1.0 + f_min / 700.0);
        let mel_max = 2595.0 * log10f(1.0 + f_max / 700.0);
        let mut bins = vec![0u64; num_filters + 2];
        for (i, bin) in bins.iter_mut().enumerate() {
            let mut mel_point = mel_min + (mel_max - mel_min) * i as f32 / (num_filters + 1) as f32;
            mel_point = 700.0 * (powf(10.0, mel_point / 2595.0) - 1.0);
            *bin = floorf(mel_point * (n_fft as f32 + 1.0) / sample_rate) as usize as u64;
        }
        bins
    }

    /// `cepstrum::mel_filterbank`.
    pub fn mel_filterbank(fft: &HipFftImpl<f32>, fft_mags: &[f32], sample_rate: f32, num_filters: usize) -> Vec<f32> {
        let mut out = vec![0.0f32; num_filters];
        fft.mel_filterbank_batch(fft_mags, fft_mags.len(), &mel_bins(sample_rate, fft_mags.len(), num_filters), &mut out)
            .expect("one row: the lengths agree and the edges are in order");
        out
    }

    /// `cepstrum::mfcc`.
    pub fn mfcc(fft: &HipFftImpl<f32>, fft_mags: &[f32], sample_rate: f32, num_mel: usize, num_coeffs: usize) -> Result<Vec<f32>, FftError> {
        let mut out = vec![0.0f32; num_coeffs];
        fft.mfcc_rows(fft_mags, fft_mags.len(), &mel_bins(sample_rate, fft_mags.len(), num_mel), num_coeffs, &mut out)?;
        Ok(out)
    }

    /// Mel energies of every frame of every row of `len` samples: `stft_magnitudes` (Hann, `ceil(len / hop)` frames per row) followed by
    /// `cepstrum::mel_filterbank` over the `win_len / 2` magnitudes of each frame, in one device call; rows * frames rows of
    /// `num_filters` energies.  The edges are `mel_bins(sample_rate, win_len / 2, num_filters)`, the crate's own.
    pub fn mel_from_audio(fft: &HipFftImpl<f32>, signals: &[f32], len: usize, sample_rate: f32, win_len: usize, hop: usize,
                          num_filters: usize) -> Result<Vec<f32>, FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        let frames = len / hop + (len % hop != 0) as usize;
        let rows = if len != 0 { signals.len() / len } else { 0 };
        let mut out = vec![0.0f32; rows * frames * num_filters];
        fft.stft_mel_rows(signals, len, None, win_len, hop, frames, &mel_bins(sample_rate, win_len / 2, num_filters), None, &mut out)?;
        Ok(out)
    }

    /// ... through `logf(e + 1e-12)` and the first `num_coeffs` outputs of `dct::dct2`: rows * frames rows of `num_coeffs` coefficients,
    /// what `cepstrum::mfcc` returns for each frame's magnitudes.
    pub fn mfcc_from_audio(fft: &HipFftImpl<f32>, signals: &[f32], len: usize, sample_rate: f32, win_len: usize, hop: usize, num_mel: usize,
                           num_coeffs: usize) -> Result<Vec<f32>, FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        let frames = len / hop + (len % hop != 0) as usize;
        let rows = if len != 0 { signals.len() / len } else { 0 };
        let mut out = vec![0.0f32; rows * frames * num_coeffs];
        fft.stft_mel_rows(signals, len, None, win_len, hop, frames, &mel_bins(sample_rate, win_len / 2, num_mel), Some(num_coeffs), &mut out)?;
        Ok(out)
    }

    /// `cepstrum::mfcc_batch`: frames of one length go to the device in one call.
    pub fn mfcc_batch(fft: &HipFftImpl<f32>, batch: &[Vec<f32>], sample_rate: f32, num_mel: usize, num_coeffs: usize) -> Result<Vec<Vec<f32>>, FftError> {
        if num_coeffs > num_mel { return if batch.is_empty() { Ok(Vec::new()) } else { Err(FftError::InvalidValue) }; }
        let mut result = vec![Vec::new(); batch.len()];
        let mut lens: Vec<usize> = batch.iter().map(|b| b.len()).collect();
        lens.sort_unstable();
        lens.dedup();
        for n in lens {
            let idx: Vec<usize> = (0..batch.len()).filter(|&j| batch[j].len() == n).collect();
            let flat: Vec<f32> = idx.iter().flat_map(|&j| batch[j].iter().copied()).collect();
            let mut out = vec![0.0f32; idx.len() * num_coeffs];
            if n != 0 {
                fft.mfcc_rows(&flat, n, &mel_bins(sample_rate, n, num_mel), num_coeffs, &mut out)?;
            } else {
                // rows without data: every energy is +0 (cepstrum.rs:51), one row stands for all of them
                let one = mfcc(fft, &[], sample_rate, num_mel, num_coeffs)?;
                for t in 0..idx.len() { out[t * num_coeffs..(t + 1) * num_coeffs].copy_from_slice(&one); }
            }
            for (t, &j) in idx.iter().enumerate() {
                result[j] = out[t * num_coeffs..(t + 1) * num_coeffs].to_vec();
            }
        }
        Ok(result)
    }
}

impl HipFftImpl<f32> {
    /// `visual::spectrogram::magnitude_to_db` (kofft visual/spectrogram.rs:96-102) of every value, with the **libm crate's** `log10f`
    /// (include/kofft_hip.h: the arithmetic contract).  No values: `EmptyInput`.
    pub fn magnitude_to_db_batch(&self, mags: &[f32], max_mag: f32, floor_db: f32, out: &mut [f32]) -> Result<(), FftError> {
        if out.len() != mags.len() { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe { kofft_hip_magnitude_to_db_f32(self.ctx, mags.as_ptr(), mags.len(), &max_mag, floor_db, out.as_mut_ptr()) })
    }

    /// `visual::spectrogram::db_scale` (spectrogram.rs:107-110) of every value.
    pub fn db_scale_batch(&self, mags: &[f32], max_mag: f32, dynamic_range: f32, out: &mut [f32]) -> Result<(), FftError> {
        if out.len() != mags.len() { return Err(FftError::MismatchedLengths); }
        status(self.ctx, unsafe { kofft_hip_db_scale_f32(self.ctx, mags.as_ptr(), mags.len(), &max_mag, dynamic_range, out.as_mut_ptr()) })
    }

    /// `frames` rows of `mags.len() / frames` magnitudes -> an RGB8 picture, three bytes per pixel.  `floor_db`: `color_from_magnitude_u8`
    /// (mode 0); `log_table`: every frame through `log_scale_bins` first, over this bin -> pixel table (`spectrogram::log_bin_map`);
    /// `image`: `[bins][frames][3]` with bin b at row bins - 1 - b (what the reference's programs build), else `[frames][bins][3]`.
    /// Viridis, Plasma and Inferno are `InvalidValue`.
    pub fn spectrogram_rgb8(&self, mags: &[f32], frames: usize, max_mag: f32, floor_db: f32, cmap: spectrogram::Colormap, log_table: Option<&[u32]>,
                            image: bool, out: &mut [u8]) -> Result<(), FftError> {
        if frames == 0 || mags.is_empty() { return Err(FftError::EmptyInput); }
        let bins = mags.len() / frames;
        if mags.len() % frames != 0 || out.len() != mags.len() * 3 || log_table.map_or(false, |t| t.len() != bins) {
            return Err(FftError::MismatchedLengths);
        }
        status(self.ctx, unsafe {
            kofft_hip_spectrogram_render_f32(self.ctx, mags.as_ptr(), frames, bins, &max_mag, 0, floor_db, cmap as c_int, 8, log_table.is_some() as c_int,
                                             image as c_int, log_table.map_or(core::ptr::null(), |t| t.as_ptr()), out.as_mut_ptr() as *mut core::ffi::c_void)
        })
    }

    /// Rows of audio -> one 8-bit picture per row in one call (include/kofft_hip.h): `stft_magnitudes` with
    /// `window::hann(win_len)`, the maximum `max` chooses, `color_from_magnitude_u8` per bin; the magnitudes stay on the device.
    /// `rgba`: four bytes per pixel, alpha 255 (`compute_frame`'s rows when `image` is false).  `out`: `rows * frames * (win_len / 2) *
    /// (3 or 4)` bytes; `max_out`: the maximum used, one per row.
    pub fn stft_picture_rows(&self, signals: &[f32], len: usize, win_len: usize, hop: usize, frames: usize, max: spectrogram::Maximum<'_>,
                             floor_db: f32, cmap: spectrogram::Colormap, rgba: bool, log_table: Option<&[u32]>, image: bool, max_out: &mut [f32],
                             out: &mut [u8]) -> Result<(), FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        let rows = if len == 0 { max_out.len() } else { signals.len() / len };
        let px = if rgba { 4 } else { 3 };
        if signals.len() != rows * len || max_out.len() != rows || out.len() != rows * frames * (win_len / 2) * px
            || log_table.map_or(false, |t| t.len() != win_len / 2) {
            return Err(FftError::MismatchedLengths);
        }
        let (max_mode, max_in) = match max {
            spectrogram::Maximum::Row => (0, core::ptr::null()),
            spectrogram::Maximum::Running => (1, core::ptr::null()),
            spectrogram::Maximum::Given(m) => {
                if m.len() != rows { return Err(FftError::MismatchedLengths); }
                (2, m.as_ptr())
            }
        };
        status(self.ctx, unsafe {
            kofft_hip_stft_picture_f32(self.ctx, signals.as_ptr(), rows, len, len, core::ptr::null(), win_len, hop, frames, max_mode, max_in,
                                       max_out.as_mut_ptr(), 0, floor_db, cmap as c_int, 8, px as c_int, log_table.is_some() as c_int, image as c_int,
                                       log_table.map_or(core::ptr::null(), |t| t.as_ptr()), out.as_mut_ptr() as *mut core::ffi::c_void)
        })
    }

    /// `true` (the default): the image layout leaves through an LDS tile; `false`: every lane stores its own bytes (the same bytes).
    pub fn set_spectrogram_transpose(&self, on: bool) -> Result<(), FftError> {
        status(self.ctx, unsafe { kofft_hip_set_spectrogram_transpose(self.ctx, on as c_int) })
    }
}

/// `kofft::visual::spectrogram`'s colour helpers (visual/spectrogram.rs:96-234) on the device.  The bin -> pixel table of the log
/// scale is computed HERE with the `libm` crate's `logf` -- a build of the reference without `std` -- and passed down; the library's
/// own helper (`kofft_hip_log_bin_map`) uses glibc's.  `log10` on the device is the libm crate's `log10f` restated
/// (`tests/spectrogram_pin.rs` pins the restatement and the four palettes against the crates).
pub mod spectrogram {
    use super::HipFftImpl;
    use kofft::fft::FftError;

    /// `Colormap` in the reference's declaration order: the values of `KOFFT_CMAP_*`.
    #[derive(Clone, Copy, Debug, PartialEq)]
    #[repr(i32)]
    pub enum Colormap { Fire = 0, Legacy = 1, Gray = 2, Viridis = 3, Plasma = 4, Inferno = 5, Rainbow = 6 }

    /// Which maximum `from_audio` colours against: the row's (`stft_magnitudes`' own: examples/spectrogram.rs, sanity-check), the running
    /// one of web-spectrogram's `State::compute_frame` (from 1e-12, updated before each pixel), or one value per row given by the caller.
    #[derive(Clone, Copy, Debug)]
    pub enum Maximum<'a> { Row, Running, Given(&'a [f32]) }

    /// spectrogram.rs:209-217 with `libm::logf`.
    pub fn map_bin_to_pixel(bin: usize, max_bin: usize) -> usize {
        if max_bin == 0 { return 0; }
        let log_max = libm::logf(max_bin as f32 + 1.0);
        let pos = libm::logf(bin as f32 + 1.0);
        libm::floorf(max_bin as f32 * pos / log_max) as usize
    }

    /// `map_bin_to_pixel(b, bins - 1)` for every bin: the table `spectrogram_rgb8` takes.
    pub fn log_bin_map(bins: usize) -> Vec<u32> {
        (0..bins).map(|b| map_bin_to_pixel(b, bins - 1).min(u32::MAX as usize) as u32).collect()
    }

    /// `magnitude_to_db` of every value of a frame set.
    pub fn magnitude_to_db(fft: &HipFftImpl<f32>, mags: &[f32], max_mag: f32, floor_db: f32) -> Result<Vec<f32>, FftError> {
        let mut out = vec![0.0f32; mags.len()];
        fft.magnitude_to_db_batch(mags, max_mag, floor_db, &mut out)?;
        Ok(out)
    }

    /// `db_scale` of every value of a frame set.
    pub fn db_scale(fft: &HipFftImpl<f32>, mags: &[f32], max_mag: f32, dynamic_range: f32) -> Result<Vec<f32>, FftError> {
        let mut out = vec![0.0f32; mags.len()];
        fft.db_scale_batch(mags, max_mag, dynamic_range, &mut out)?;
        Ok(out)
    }

    /// The picture the reference's `examples/spectrogram.rs` builds pixel by pixel: `[bins][frames][3]`, low frequencies at the bottom.
    pub fn render_rgb8(fft: &HipFftImpl<f32>, mags: &[Vec<f32>], max_mag: f32, floor_db: f32, cmap: Colormap, log_scale: bool) -> Result<Vec<u8>, FftError> {
        let frames = mags.len();
        let bins = mags.first().map_or(0, |f| f.len());
        if mags.iter().any(|f| f.len() != bins) { return Err(FftError::MismatchedLengths); }
        let flat: Vec<f32> = mags.iter().flat_map(|f| f.iter().copied()).collect();
        let mut out = vec![0u8; flat.len() * 3];
        let table = if log_scale { Some(log_bin_map(bins)) } else { None };
        fft.spectrogram_rgb8(&flat, frames, max_mag, floor_db, cmap, table.as_deref(), true, &mut out)?;
        Ok(out)
    }

    /// Audio -> pictures in one call: what examples/spectrogram.rs and sanity-check do with `stft_magnitudes`, its maximum and
    /// `color_from_magnitude_u8` (`Maximum::Row`, `image` true), and what web-spectrogram's `compute_frame` does a frame at a time
    /// (`Maximum::Running`, `rgba` true, `image` false, Rainbow, a floor of -80 dB), for `signals.len() / len` rows at once; the
    /// magnitudes never reach the caller.  Returns (the pictures, `ceil(len / hop)` frames each, and the maximum used per row).
    pub fn from_audio(fft: &HipFftImpl<f32>, signals: &[f32], len: usize, win_len: usize, hop: usize, max: Maximum<'_>, floor_db: f32,
                      cmap: Colormap, rgba: bool, log_scale: bool, image: bool) -> Result<(Vec<u8>, Vec<f32>), FftError> {
        if hop == 0 { return Err(FftError::InvalidHopSize); }
        if len == 0 || signals.len() % len != 0 { return Err(FftError::MismatchedLengths); }
        let (rows, frames, bins) = (signals.len() / len, (len + hop - 1) / hop, win_len / 2);
        let mut out = vec![0u8; rows * frames * bins * if rgba { 4 } else { 3 }];
        let mut max_out = vec![0.0f32; rows];
        let table = if log_scale { Some(log_bin_map(bins)) } else { None };
        fft.stft_picture_rows(signals, len, win_len, hop, frames, max, floor_db, cmap, rgba, table.as_deref(), image, &mut max_out, &mut out)?;
        Ok((out, max_out))
    }
}

/// `kofft::hartley` (hartley.rs:12-57) on the device: the reference's three functions with a context in front.
pub mod hartley {
    use super::HipFftImpl;

    /// `hartley::dht`.
    pub fn dht(fft: &HipFftImpl<f32>, input: &[f32]) -> Vec<f32> {
        let mut out = vec![0.0f32; input.len()];
        fft.dht_batch(input, input.len(), &mut out).expect("one row: the lengths agree");
        out
    }

    /// `hartley::batch`: every row replaced by its transform; rows of one length go to the device in one call.
    pub fn batch(fft: &HipFftImpl<f32>, batches: &mut [Vec<f32>]) {
        let mut lens: Vec<usize> = batches.iter().map(|b| b.len()).filter(|&n| n != 0).collect();
        lens.sort_unstable();
        lens.dedup();
        for n in lens {
            let idx: Vec<usize> = (0..batches.len()).filter(|&j| batches[j].len() == n).collect();
            let flat: Vec<f32> = idx.iter().flat_map(|&j| batches[j].iter().copied()).collect();
            let mut out = vec![0.0f32; flat.len()];
            fft.dht_batch(&flat, n, &mut out).expect("rows of one length");
            for (t, &j) in idx.iter().enumerate() {
                batches[j].copy_from_slice(&out[t * n..(t + 1) * n]);
            }
        }
    }

    /// `hartley::multi_channel`: `batch`.
    pub fn multi_channel(fft: &HipFftImpl<f32>, channels: &mut [Vec<f32>]) {
        batch(fft, channels)
    }
}

/// `kofft::window` / `kofft::window_more` beyond `hann` (window.rs:31-61, window_more.rs:13-64), generated by the library's host
/// recipes bit for bit; no device is involved.
pub mod window {
    use core::ffi::c_int;

    fn make(kind: c_int, len: usize, param: f32) -> Vec<f32> {
        let mut w = vec![0.0f32; len];
        let rc = unsafe { super::kofft_hip_window_f32(kind, len, param, w.as_mut_ptr()) };
        assert_eq!(rc, 0, "kofft_hip_window_f32 status {rc}");
        w
    }
    pub fn hamming(len: usize) -> Vec<f32> { make(0, len, 0.0) }
    pub fn blackman(len: usize) -> Vec<f32> { make(1, len, 0.0) }
    /// Panics at `len == 0`, where the reference underflows `len - 1`.
    pub fn kaiser(len: usize, beta: f32) -> Vec<f32> { make(2, len, beta) }
    pub fn tukey(len: usize, alpha: f32) -> Vec<f32> { make(3, len, alpha) }
    pub fn bartlett(len: usize) -> Vec<f32> { make(4, len, 0.0) }
    pub fn bohman(len: usize) -> Vec<f32> { make(5, len, 0.0) }
    pub fn nuttall(len: usize) -> Vec<f32> { make(6, len, 0.0) }
}

/// `stft::parallel` (kofft stft.rs:232-263) across `ngpu` devices of this process: frames are the parallel unit, device
/// `r` computes `[r*ceil(F/G), ...)`; `allgather` adds the RCCL all-gather of BASELINE config #4.  Same checks as
/// `stft::stft` (stft.rs:83-87).  One call: contexts are created and torn down inside (see `HipMulti` to keep them).
pub fn stft_multi(ngpu: usize, signal: &[f32], window: &[f32], hop_size: usize, output: &mut [Vec<Complex32>], allgather: bool)
    -> Result<(), FftError> {
    let (frames, wl) = (output.len(), window.len());
    let mut flat = vec![Complex32::new(0.0, 0.0); frames * wl];
    let rc = unsafe {
        kofft_hip_stft_f32_multi(ngpu as c_int, signal.as_ptr(), signal.len(), window.as_ptr(), wl, hop_size,
                                 flat.as_mut_ptr() as *mut f32, frames, allgather as c_int)
    };
    status(core::ptr::null(), rc)?;
    for (f, frame) in output.iter_mut().enumerate() {
        frame.clear();
        frame.extend_from_slice(&flat[f * wl..(f + 1) * wl]);
    }
    Ok(())
}

/// Handle form of the above: per-device contexts, buffers and RCCL communicators live as long as the value.
pub struct HipMulti {
    h: *mut KofftHipMulti,
}

impl HipMulti {
    pub fn new(ngpu: usize) -> Result<Self, FftError> {
        let mut h = core::ptr::null_mut();
        status(core::ptr::null(), unsafe { kofft_hip_multi_create(ngpu as c_int, core::ptr::null(), &mut h) })?;
        Ok(Self { h })
    }

    pub fn stft_contiguous(&self, signal: &[f32], window: &[f32], hop_size: usize, out: &mut [Complex32], allgather: bool)
        -> Result<(), FftError> {
        let frames = if window.is_empty() { 0 } else { out.len() / window.len() };
        let rc = unsafe {
            kofft_hip_multi_stft_f32(self.h, signal.as_ptr(), signal.len(), window.as_ptr(), window.len(), hop_size,
                                     out.as_mut_ptr() as *mut f32, frames, allgather as c_int, core::ptr::null_mut())
        };
        if rc < 0 {
            let msg = unsafe { std::ffi::CStr::from_ptr(kofft_hip_multi_last_error(self.h)) }.to_string_lossy().into_owned();
            panic!("kofft-hip multi-GPU error {rc}: {msg}");
        }
        status(core::ptr::null(), rc)
    }

    fn check(&self, rc: c_int) -> Result<(), FftError> {
        if rc < 0 {
            let msg = unsafe { std::ffi::CStr::from_ptr(kofft_hip_multi_last_error(self.h)) }.to_string_lossy().into_owned();
            panic!("kofft-hip multi-GPU error {rc}: {msg}");
        }
        status(core::ptr::null(), rc)
    }

    /// `fft::batch` (fft.rs:2156-2175) over `batch` contiguous transforms of length `n`, the batch in G contiguous blocks.
    pub fn fft_batch_c32(&self, data: &mut [Complex32], n: usize, inverse: bool) -> Result<(), FftError> {
        let batch = if n == 0 { 0 } else { data.len() / n };
        self.check(unsafe { kofft_hip_multi_fft_c32(self.h, data.as_mut_ptr() as *mut f32, n, batch, inverse as c_int) })
    }
    pub fn fft_batch_c64(&self, data: &mut [Complex64], n: usize, inverse: bool) -> Result<(), FftError> {
        let batch = if n == 0 { 0 } else { data.len() / n };
        self.check(unsafe { kofft_hip_multi_fft_c64(self.h, data.as_mut_ptr() as *mut f64, n, batch, inverse as c_int) })
    }
    /// `rfft_direct` (rfft.rs:425-465) on every row of `n` reals (optional window product first), rows sharded over the devices.
    pub fn rfft_batch(&self, input: &[f32], out: &mut [Complex32], window: Option<&[f32]>, n: usize) -> Result<(), FftError> {
        let batch = if n == 0 { 0 } else { input.len() / n };
        if out.len() != batch * (n / 2 + 1) || window.map_or(false, |w| w.len() != n) {
            return Err(FftError::MismatchedLengths);
        }
        let w = window.map_or(core::ptr::null(), |w| w.as_ptr());
        self.check(unsafe { kofft_hip_multi_rfft_f32(self.h, input.as_ptr(), out.as_mut_ptr() as *mut f32, w, n, batch) })
    }
    /// (first, count) of the `total` units device `rank` owns.
    pub fn shard(&self, total: usize, rank: usize) -> (usize, usize) {
        let (mut f, mut c) = (0usize, 0usize);
        unsafe { kofft_hip_multi_shard(self.h, total, rank as c_int, &mut f, &mut c) };
        (f, c)
    }
    /// (first_sample, count) of the signal slice device `rank` needs for its frames (block + halo).
    pub fn stft_slice(&self, len: usize, win_len: usize, hop: usize, frames: usize, rank: usize) -> (usize, usize) {
        let (mut f, mut c) = (0usize, 0usize);
        unsafe { kofft_hip_multi_stft_slice(self.h, len, win_len, hop, frames, rank as c_int, &mut f, &mut c) };
        (f, c)
    }
    /// Device-resident forms: `d_*[r]` is a pointer valid on device r; asynchronous, `synchronize()` waits.
    ///
    /// # Safety
    /// The pointers must be device allocations of the sizes include/kofft_hip.h states for each entry.
    pub unsafe fn fft_c32_dev(&self, d_data: &[*mut f32], n: usize, batch: usize, inverse: bool) -> Result<(), FftError> {
        self.check(kofft_hip_multi_fft_c32_dev(self.h, d_data.as_ptr(), n, batch, inverse as c_int))
    }
    /// # Safety
    /// As `fft_c32_dev`.
    pub unsafe fn fft_c64_dev(&self, d_data: &[*mut f64], n: usize, batch: usize, inverse: bool) -> Result<(), FftError> {
        self.check(kofft_hip_multi_fft_c64_dev(self.h, d_data.as_ptr(), n, batch, inverse as c_int))
    }
    /// # Safety
    /// As `fft_c32_dev`.
    pub unsafe fn rfft_dev(&self, d_in: &[*const f32], d_out: &[*mut f32], d_window: Option<&[*const f32]>, n: usize, batch: usize)
        -> Result<(), FftError> {
        let w = d_window.map_or(core::ptr::null(), |w| w.as_ptr());
        self.check(kofft_hip_multi_rfft_f32_dev(self.h, d_in.as_ptr(), d_out.as_ptr(), w, n, batch))
    }
    /// `d_out[r]` null on entry = a buffer owned by the handle is used and written back into the slice.
    ///
    /// # Safety
    /// As `fft_c32_dev`.
    pub unsafe fn stft_dev(&self, d_signal: &[*const f32], len: usize, d_window: &[*const f32], win_len: usize, hop: usize,
                           frames: usize, allgather: bool, d_out: &mut [*mut f32]) -> Result<(), FftError> {
        self.check(kofft_hip_multi_stft_f32_dev(self.h, d_signal.as_ptr(), len, d_window.as_ptr(), win_len, hop, frames,
                                                allgather as c_int, d_out.as_mut_ptr()))
    }
    pub fn synchronize(&self) -> Result<(), FftError> {
        self.check(unsafe { kofft_hip_multi_synchronize(self.h) })
    }
    /// 1 = RCCL (grouped in-place ncclAllGather), 2 = direct (peer copies on a stream per peer)
    pub fn set_gather(&self, mode: i32) -> Result<(), FftError> {
        self.check(unsafe { kofft_hip_multi_set_gather(self.h, mode as c_int) })
    }
    /// the form the last call's exchange ran (0: it had none)
    pub fn last_gather(&self) -> i32 {
        let mut last: c_int = 0;
        unsafe { kofft_hip_multi_gather_mode(self.h, std::ptr::null_mut(), &mut last) };
        last as i32
    }
    pub fn last_timing(&self) -> MultiTiming {
        let mut t = MultiTiming::default();
        unsafe {
            kofft_hip_multi_last_timing_ex(self.h, &mut t.upload_ms, &mut t.kernel_ms, &mut t.gather_ms, &mut t.download_ms, &mut t.wall_ms)
        };
        t
    }
}

impl Drop for HipMulti {
    fn drop(&mut self) {
        unsafe { kofft_hip_multi_destroy(self.h) };
    }
}

#[allow(dead_code)]
fn _assert_traits() {
    fn is_fft_impl<F: FftImpl<f32>>() {}
    is_fft_impl::<HipFftImpl<f32>>();
    let _ = core::mem::size_of::<*mut c_void>();
}
