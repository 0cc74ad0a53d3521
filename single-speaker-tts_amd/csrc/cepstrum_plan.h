// Mel-frequency cepstral coefficients, host side: the DCT table and the argument checks of tts_mfcc.  Plain C++ (no HIP, no
// handle): cepstrum.hip includes it, and tests/dtw_check.cpp compiles it alone.
//   calculate_mfccs             reference audio/features.py:89-113: librosa.feature.mfcc(S=mel_spec, n_mfcc=n), which with S given is
//                               scipy.fftpack.dct(S, axis=0, type=2, norm='ortho')[:n_mfcc]
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace tts {

constexpr int MFCC_MAX_MELS = 1024;
constexpr int MFCC_UTTS = 64;   // utterances per launch: their lengths travel by value

// The orthonormal DCT-II, in double: d[k][n] = sqrt(2 / n_mels) cos(pi k (2 n + 1) / (2 n_mels)), row 0 times 1 / sqrt(2).
// Laid out [n][k] (n_mels rows of n_mfcc): the lanes of the kernel run along k.
inline std::vector<double> mfcc_table(int n_mels, int n_mfcc) {
    std::vector<double> tab((size_t)n_mels * n_mfcc);
    const double pi = 3.14159265358979323846, scale = std::sqrt(2.0 / (double)n_mels);
    for (int n = 0; n < n_mels; ++n)
        for (int k = 0; k < n_mfcc; ++k) {
            double v = scale * std::cos(pi * (double)k * (double)(2 * n + 1) / (double)(2 * n_mels));
            if (k == 0) v *= 1.0 / std::sqrt(2.0);
            tab[(size_t)n * n_mfcc + k] = v;
        }
    return tab;
}

// The checks of tts_mfcc, in the order the header lists them; an empty string: the call is legal.  n_frames: host lengths or null
// (all T).
inline std::string mfcc_check(bool have_ptrs, int B, int T, int n_mels, int row_stride, const int32_t* n_frames, int n_mfcc) {
    if (!have_ptrs) return "a NULL pointer";
    if (B < 1 || T < 1 || n_mels < 1 || n_mfcc < 1) return "need B, T, n_mels, n_mfcc >= 1";
    if (n_mels > MFCC_MAX_MELS) return "n_mels is larger than " + std::to_string(MFCC_MAX_MELS);
    if (n_mfcc > n_mels) return "n_mfcc > n_mels";
    if (row_stride < n_mels) return "row_stride < n_mels";
    return lengths_refusal("n_frames", n_frames, B, "T", T);
}

}  // namespace tts
