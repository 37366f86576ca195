//! Reference pins for the spectrogram colour helpers: the REAL `libm` crate's `log10f` against the bits the library's restatement
//! (kofft_amd/csrc/libm_log10f.hip.h, equal bit for bit to tests/spectrogram_oracle.py on the device and on the host) returns on a
//! fixed list of arguments, and the four implemented palettes of kofft's own `map_color_u8` against `kofft_hip_map_color_u8`.
//!
//! The build image of this repository has no Rust toolchain, so this file has never been compiled there.  On any box with cargo
//! and the built library:
//!
//!     cd integration/rust/kofft-hip && cargo test --test spectrogram_pin -- --nocapture
//!
//! The list: 1, 0.5, the powers of ten 1e-1 .. 1e-10 (log10f must return -k exactly where `10f32.powi(-k)` is the argument), both
//! neighbours of 1, both sides of the reduction's split at sqrt(2)/2 and sqrt(2), the smallest subnormal, a middle and the largest
//! one, the smallest normal, 10, the largest finite value, 0.3 and pi.
use kofft::visual::spectrogram::{map_color_u8, Colormap};

extern "C" {
    fn kofft_hip_map_color_u8(t: f32, cmap: core::ffi::c_int, rgb: *mut u8) -> core::ffi::c_int;
}

const LOG10F: [(u32, u32); 24] = [
    (0x3f800000, 0x00000000), (0x3f000000, 0xbe9a209b), (0x3dcccccd, 0xbf800000), (0x3c23d70a, 0xc0000000), (0x3a83126f, 0xc0400000),
    (0x38d1b717, 0xc0800000), (0x3727c5ac, 0xc0a00000), (0x358637bd, 0xc0c00000), (0x33d6bf95, 0xc0e00000), (0x322bcc77, 0xc1000000),
    (0x2edbe6ff, 0xc1200000), (0x3f7fffff, 0xb2de5bd9), (0x3f800001, 0x335e5bd8), (0x3f3504f3, 0xbe1a209b), (0x3f3504f2, 0xbe1a209e),
    (0x3fb504f3, 0x3e1a209a), (0x00000001, 0xc23369f4), (0x00400000, 0xc218ec59), (0x007fffff, 0xc217b818), (0x00800000, 0xc217b818),
    (0x41200000, 0x3f800000), (0x7f7fffff, 0x421a209b), (0x3e99999a, 0xbf05db61), (0x40490fdb, 0x3efe8a6e),
];

#[test]
fn the_crates_log10f_is_the_restatement() {
    for &(x, want) in &LOG10F {
        let got = libm::log10f(f32::from_bits(x)).to_bits();
        assert_eq!(got, want, "log10f({:#010x}) = {:#010x}, the restatement gives {:#010x}", x, got, want);
    }
    assert_eq!(libm::log10f(0.0), f32::NEG_INFINITY);
    assert!(libm::log10f(-1.0).is_nan() && libm::log10f(f32::NAN).is_nan());
    assert_eq!(libm::log10f(f32::INFINITY), f32::INFINITY);
}

#[test]
fn the_four_palettes_are_the_crates() {
    for (cmap, id) in [(Colormap::Fire, 0), (Colormap::Legacy, 1), (Colormap::Gray, 2), (Colormap::Rainbow, 6)] {
        let ts = (0..=1024).map(|i| i as f32 / 1024.0).chain([f32::NAN, -1.0, 2.0, 0.9]);
        for t in ts {
            let mut rgb = [0u8; 3];
            assert_eq!(unsafe { kofft_hip_map_color_u8(t, id, rgb.as_mut_ptr()) }, 0);
            assert_eq!(rgb, map_color_u8(t, cmap), "{:?} at t = {}", cmap, t);
        }
    }
    let mut rgb = [0u8; 3];
    for id in [3, 4, 5] {
        assert_eq!(unsafe { kofft_hip_map_color_u8(0.5, id, rgb.as_mut_ptr()) }, 6, "the colorous palettes are not implemented");
    }
}
