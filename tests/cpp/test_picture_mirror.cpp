// Audio -> spectrogram pictures in one call through the C++ host mirror (include/kofft_hip.hpp: stft_picture, stft_picture_dev): what
// examples/spectrogram.rs does -- stft_magnitudes, its maximum, a colour per bin -- as ONE call against the mirror's two-call chain
// (stft_magnitudes_rows, then spectrogram_render per row), byte for byte; the given maximum, the RGBA pixel, the running maximum's
// final value, and the mirror's argument errors.  Exit status 0 and " 0 failed" when every check passes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/kofft_hip.hpp"

using namespace kofft;
static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

template <typename Pixel>
static void against_the_chain(const HipFftImpl<float> &fft, const std::vector<float> &x, size_t rows, size_t win_len, size_t hop, int layout)
{
    const size_t len = x.size() / rows, frames = (len + hop - 1) / hop, bins = win_len / 2;
    std::vector<float> mags, max_mag, max_out, none;
    CHECK(stft_magnitudes_rows(x, rows, win_len, hop, mags, max_mag, fft).is_ok());
    std::vector<Pixel> chain(rows * frames * bins * 3), one(chain.size()), row(frames * bins * 3), given(chain.size());
    const std::vector<uint32_t> no_table;
    for (size_t r = 0; r < rows; ++r) {
        const std::vector<float> m(mags.begin() + r * frames * bins, mags.begin() + (r + 1) * frames * bins);
        CHECK(fft.spectrogram_render(m, frames, max_mag[r], 0, -80.0f, KOFFT_CMAP_RAINBOW, 0, layout, no_table, row).is_ok());
        std::memcpy(chain.data() + r * row.size(), row.data(), row.size() * sizeof(Pixel));
    }
    CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_out, 0, -80.0f, KOFFT_CMAP_RAINBOW, 3, 0, layout, no_table, one).is_ok());
    CHECK(std::memcmp(one.data(), chain.data(), chain.size() * sizeof(Pixel)) == 0);
    CHECK(max_out.size() == rows && std::memcmp(max_out.data(), max_mag.data(), rows * sizeof(float)) == 0);
    std::vector<float> copy;
    CHECK(fft.stft_picture(x, rows, win_len, hop, 2, max_out, copy, 0, -80.0f, KOFFT_CMAP_RAINBOW, 3, 0, layout, no_table, given).is_ok());
    CHECK(std::memcmp(given.data(), one.data(), one.size() * sizeof(Pixel)) == 0);
    CHECK(std::memcmp(copy.data(), max_out.data(), rows * sizeof(float)) == 0);
}

int main()
{
    HipFftImpl<float> fft;
    const size_t rows = 3, len = 3000, win_len = 256, hop = 64, frames = (len + hop - 1) / hop, bins = win_len / 2;
    std::vector<float> x(rows * len);
    for (size_t i = 0; i < x.size(); ++i) x[i] = std::sin(0.013f * (float)i) * (1.0f + (float)(i % len) / 300.0f) + 0.3f * std::cos(1.7f * (float)i);
    for (int layout : {0, 1}) {
        against_the_chain<uint8_t>(fft, x, rows, win_len, hop, layout);
        against_the_chain<uint16_t>(fft, x, rows, win_len, hop, layout);
    }
    const std::vector<uint32_t> no_table;
    std::vector<float> none, max_row, max_run;
    {   // RGBA: alpha 255, the colours of channels 3; compute_frame's layout (frames, 4 channels, Rainbow, a floor of -80 dB)
        std::vector<uint8_t> three(rows * frames * bins * 3), four(rows * frames * bins * 4);
        for (int max_mode : {0, 1}) {
            CHECK(fft.stft_picture(x, rows, win_len, hop, max_mode, none, max_row, 0, -80.0f, KOFFT_CMAP_RAINBOW, 3, 0, 0, no_table, three).is_ok());
            CHECK(fft.stft_picture(x, rows, win_len, hop, max_mode, none, max_run, 0, -80.0f, KOFFT_CMAP_RAINBOW, 4, 0, 0, no_table, four).is_ok());
            bool same = true;
            for (size_t p = 0; p < rows * frames * bins; ++p)
                same = same && four[4 * p + 3] == 255 && std::memcmp(&four[4 * p], &three[3 * p], 3) == 0;
            CHECK(same);
            CHECK(std::memcmp(max_row.data(), max_run.data(), rows * sizeof(float)) == 0);
        }
        // the running maximum ends at the row's maximum (above the 1e-12 seed here), and a first pixel is coloured against itself: t == 1
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 0, -80.0f, KOFFT_CMAP_RAINBOW, 4, 0, 0, no_table, four).is_ok());
        std::vector<uint8_t> run(four.size());
        CHECK(fft.stft_picture(x, rows, win_len, hop, 1, none, max_run, 0, -80.0f, KOFFT_CMAP_RAINBOW, 4, 0, 0, no_table, run).is_ok());
        CHECK(std::memcmp(max_row.data(), max_run.data(), rows * sizeof(float)) == 0 && max_run[0] > 1e-12f);
        for (size_t r = 0; r < rows; ++r) {
            const uint8_t *first = &run[r * frames * bins * 4];
            CHECK(first[0] == 255 && first[1] == 255 && first[2] == 255 && first[3] == 255);  // Rainbow's last stop
        }
        CHECK(std::memcmp(run.data(), four.data(), run.size()) != 0);  // an earlier pixel saw a smaller maximum
    }
    {   // a caller's window, more frames than the signal fills, and the table of the log scale
        std::vector<float> win(win_len);
        for (size_t i = 0; i < win_len; ++i) win[i] = 0.54f - 0.46f * std::cos(6.2831853f * (float)i / (float)(win_len - 1));
        std::vector<uint32_t> table(bins);
        CHECK(kofft_hip_log_bin_map(bins, table.data()) == 0);
        std::vector<uint8_t> out(rows * (frames + 2) * bins * 3);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 1, 70.0f, KOFFT_CMAP_FIRE, 3, 1, 1, table, out, win, frames + 2).is_ok());
        CHECK(fft.stft_picture(x, rows, win_len, hop, 1, none, max_row, 1, 70.0f, KOFFT_CMAP_FIRE, 3, 1, 1, table, out, win, frames + 2).unwrap_err() ==
              FftError::InvalidValue);
    }
    {   // the mirror's errors, in its order
        std::vector<uint8_t> out(rows * frames * bins * 3);
        CHECK(fft.stft_picture(x, rows, win_len, 0, 0, none, max_row, 0, -80.0f, 0, 3, 0, 1, no_table, out).unwrap_err() == FftError::InvalidHopSize);
        CHECK(fft.stft_picture(x, 7, win_len, hop, 0, none, max_row, 0, -80.0f, 0, 3, 0, 1, no_table, out).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 0, -80.0f, 0, 5, 0, 1, no_table, out).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 2, none, max_row, 0, -80.0f, 0, 3, 0, 1, no_table, out).unwrap_err() == FftError::MismatchedLengths);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 0, -80.0f, 0, 3, 0, 1, no_table, out, {}, frames - 1).unwrap_err() ==
              FftError::MismatchedLengths);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 0, -80.0f, KOFFT_CMAP_VIRIDIS, 3, 0, 1, no_table, out).unwrap_err() ==
              FftError::InvalidValue);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 3, none, max_row, 0, -80.0f, 0, 3, 0, 1, no_table, out).unwrap_err() == FftError::InvalidValue);
        std::vector<uint16_t> wide(rows * frames * bins * 4);
        CHECK(fft.stft_picture(x, rows, win_len, hop, 0, none, max_row, 0, -80.0f, 0, 4, 0, 1, no_table, wide).unwrap_err() == FftError::InvalidValue);
        CHECK(fft.stft_picture_dev(nullptr, 0, 0, 0, nullptr, win_len, hop, 0, 0, nullptr, nullptr, 0, -80.0f, 0, 8, 3, 0, 1, no_table, nullptr).is_ok());
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
