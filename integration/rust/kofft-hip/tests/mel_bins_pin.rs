//! Reference pin for the mel filter edges: the REAL `libm` crate's `log10f` / `powf` (what kofft's cepstrum.rs:38-50 calls, here
//! through `kofft_hip::cepstrum::mel_bins`) against the library's glibc-based helper `kofft_hip_mel_bins_f32`.
//!
//! The build image of this repository has no Rust toolchain, so this file has never been compiled there.  On any box with cargo
//! and the built library:
//!
//!     cd integration/rust/kofft-hip && cargo test --test mel_bins_pin -- --nocapture
//!
//! The seven settings of tests/test_mel_cpu.py keep every exact edge at least 1.5e-3 away from an integer: there the two must
//! agree, and a failure names the setting and the edge.  The odd `n_fft` settings are the known unpinned case -- the last edge is
//! the integer (n_fft + 1) / 2 in exact arithmetic, so its floor hangs on the last bit of both functions -- and are only reported.
//! Everything after the edges (the sums, logf, dct2) is pinned bit for bit by the repository's own tests, whatever the edges are.
extern "C" {
    fn kofft_hip_mel_bins_f32(sample_rate: f32, n_fft: usize, num_filters: usize, bins: *mut u64) -> core::ffi::c_int;
}

fn library_bins(rate: f32, n_fft: usize, filters: usize) -> Vec<u64> {
    let mut bins = vec![0u64; filters + 2];
    assert_eq!(unsafe { kofft_hip_mel_bins_f32(rate, n_fft, filters, bins.as_mut_ptr()) }, 0);
    bins
}

#[test]
fn the_crates_edges_equal_the_librarys_where_they_are_pinned() {
    for &(rate, n_fft, filters) in &[(16000.0f32, 32usize, 8usize), (16000.0, 256, 26), (16000.0, 512, 40), (48000.0, 512, 40),
                                     (22050.0, 1024, 128), (8000.0, 8, 40), (16000.0, 64, 13)] {
        assert_eq!(kofft_hip::cepstrum::mel_bins(rate, n_fft, filters), library_bins(rate, n_fft, filters), "({rate}, {n_fft}, {filters})");
    }
    for &(rate, n_fft, filters) in &[(16000.0f32, 33usize, 8usize), (16000.0, 257, 40)] {
        let (a, b) = (kofft_hip::cepstrum::mel_bins(rate, n_fft, filters), library_bins(rate, n_fft, filters));
        println!("({rate}, {n_fft}, {filters}): last edge crate {} library {}{}", a[filters + 1], b[filters + 1],
                 if a == b { "" } else { "  <- differ: the unpinned case" });
    }
}
