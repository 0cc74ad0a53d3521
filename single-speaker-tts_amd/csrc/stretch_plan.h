// Speaking rate, host side: the frame count of a stretched utterance and the argument checks of the stretch entry points.
// Plain C++ (no HIP, no handle): stretch.hip and the pipeline include it, and tests/stretch_check.cpp compiles it alone.
//   time_stretch                reference audio/effects.py:46-88 (librosa 0.6 phase_vocoder, of which only np.abs is kept)
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstdint>
#include <string>

namespace tts {

constexpr double STRETCH_RATE_MIN = 0.25, STRETCH_RATE_MAX = 4.0;

// a NaN fails both comparisons
inline bool stretch_rate_ok(double rate) { return rate >= STRETCH_RATE_MIN && rate <= STRETCH_RATE_MAX; }

// len(np.arange(0, n, rate, dtype=float)) = ceil(n / rate), the division and the ceil in double as numpy makes them.
// At most 4 n for the rates stretch_rate_ok admits; 0 for n < 1.
inline long long stretched_frames(int n, double rate) {
    if (n < 1) return 0;
    return (long long)std::ceil((double)n / rate);
}

// The checks of tts_stretch_magnitudes / tts_stretch_rows, in the order the header lists them; an empty string: the call is
// legal.  n_frames: host lengths or null (all T).  have_ptrs: the data pointers are not NULL.
inline std::string stretch_check(bool have_ptrs, int B, int F, int T, int row_stride, const int32_t* n_frames, double rate, int T_out) {
    if (!have_ptrs) return "a NULL pointer";
    if (!stretch_rate_ok(rate)) return "the rate must be finite and lie in [0.25, 4]";
    if (B < 1 || F < 1 || T < 1) return "need B, F, T >= 1";
    if (row_stride < F) return "row_stride < F";
    long long longest = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_frames ? n_frames[b] : T;
        const std::string why = length_refusal("n_frames", b, n, "T", T);
        if (!why.empty()) return why;
        const long long m = stretched_frames(n, rate);
        longest = m > longest ? m : longest;
    }
    if ((long long)T_out < longest)
        return "T_out = " + std::to_string(T_out) + " is smaller than the longest stretched utterance, " + std::to_string(longest) + " frames";
    return std::string();
}

}  // namespace tts
