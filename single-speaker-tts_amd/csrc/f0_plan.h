// F0 tracking (YIN), host side: the frames of a waveform, the first sample of a frame's span, the frames a workgroup owns and
// the LDS it asks for, the lanes' lag slots and the argument checks of tts_f0 and tts_f0_compare.  Plain C++ (no HIP, no
// handle): f0.hip includes it, and tests/f0_check.cpp compiles it alone.
//
// Frame t of an utterance sits at sample t * hop; its span is the W + tau_max samples from f0_first_sample(t, hop, W, tau_max).
// A workgroup owns `frames` consecutive frames of one utterance and stages their common span -- f0_span(W, tau_max, hop, frames)
// samples, as doubles -- in LDS once, beside two tables of `frames` rows of f0_row_stride(tau_max) doubles: the difference
// function (then its normalised form) and the running sums of the normalisation.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int F0_MAX_WINDOW = 2048;
constexpr int F0_MAX_LAG = 1024;
constexpr int F0_LANES = 256;                          // lanes of a workgroup
constexpr int F0_SLOTS = F0_MAX_LAG / F0_LANES;        // lags a lane owns at most: tau = 1 + lane + slot * F0_LANES
constexpr int F0_MAX_GROUP = 8;                        // frames a workgroup owns at most
constexpr int F0_UTTS = 64;                            // utterances per launch: their lengths travel by value
constexpr size_t F0_LDS_BUDGET = 48 * 1024;            // bytes of LDS a workgroup may ask for: three workgroups share a compute unit

// (constexpr: the kernel calls these too)
constexpr int f0_frames(int n, int hop) { return 1 + n / hop; }
constexpr long long f0_first_sample(long long t, int hop, int W, int tau_max) { return t * hop - (W + tau_max) / 2; }
// the slots of a lane that can hold a lag at all: ceil(tau_max / F0_LANES)
constexpr int f0_slots(int tau_max) { return (tau_max + F0_LANES - 1) / F0_LANES; }
// a row of the two tables holds the lags 0 .. tau_max; an odd count of doubles puts the rows of a group on different banks
constexpr int f0_row_stride(int tau_max) { return (tau_max + 1) | 1; }
constexpr size_t f0_span(int W, int tau_max, int hop, int frames) { return (size_t)W + tau_max + (size_t)(frames - 1) * hop; }
constexpr size_t f0_lds_bytes(int W, int tau_max, int hop, int frames) {
    return sizeof(double) * (f0_span(W, tau_max, hop, frames) + 2 * (size_t)frames * f0_row_stride(tau_max));
}
// the most frames, up to F0_MAX_GROUP, whose span and tables fit the budget (one frame always does: 40 KiB at the limits)
inline int f0_group_frames(int W, int tau_max, int hop) {
    int frames = 1;
    while (frames < F0_MAX_GROUP && f0_lds_bytes(W, tau_max, hop, frames + 1) <= F0_LDS_BUDGET) ++frames;
    return frames;
}
inline int f0_groups(int T, int frames) { return (T + frames - 1) / frames; }

// The lag bounds of the Python surface: tau_min = max(2, int(sr // fmax)), tau_max = ceil(sr / fmin).
inline int f0_tau_min(double sr, double fmax) {
    const double t = std::floor(sr / fmax);
    return t < 2.0 ? 2 : t > 2147483647.0 ? 2147483647 : (int)t;
}
inline int f0_tau_max(double sr, double fmin) {
    const double t = std::ceil(sr / fmin);
    return t > 2147483647.0 ? 2147483647 : t < 0.0 ? 0 : (int)t;
}

// The checks of tts_f0, in the order the header lists them.  An empty string: the call is legal.  *unsupported is set where the
// refusal is a window or a lag beyond the limits (TTS_ERR_UNSUPPORTED), cleared otherwise (TTS_ERR_INVALID).  n_samples: host
// lengths or null (all N).
inline std::string f0_check(bool have_ptrs, int B, int N, const int32_t* n_samples, double sampling_rate, int hop, int W, int tau_min, int tau_max,
                            double threshold, bool* unsupported) {
    *unsupported = false;
    if (!have_ptrs) return "a NULL pointer (wav and f0 are required)";
    if (B < 1 || N < 1 || hop < 1) return "need B, N, hop >= 1";
    if (N / hop >= 2147483647) return "1 + N / hop frames do not fit an int";
    const std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N);
    if (!bad.empty()) return bad;
    if (!(std::isfinite(sampling_rate) && sampling_rate > 0.0)) return "the sampling rate must be finite and positive";
    if (std::isnan(threshold)) return "the threshold is NaN";
    if (W < 1 || W > F0_MAX_WINDOW) {
        *unsupported = true;
        return "W = " + std::to_string(W) + " is not in 1 .. tts_f0_max_window() = " + std::to_string(F0_MAX_WINDOW);
    }
    if (tau_min < 2 || tau_min > tau_max || tau_max > F0_MAX_LAG) {
        *unsupported = true;
        return "the lags " + std::to_string(tau_min) + " .. " + std::to_string(tau_max) + " are not 2 <= tau_min <= tau_max <= tts_f0_max_lag() = " +
               std::to_string(F0_MAX_LAG);
    }
    return std::string();
}

// The checks of tts_f0_compare (all TTS_ERR_INVALID).
inline std::string f0_compare_check(bool have_ptrs, int Ta, int Tb, int rows, int B) {
    if (!have_ptrs) return "a NULL pointer (f0_a, f0_b, path, counts and sums are required)";
    if (B < 1 || Ta < 1 || Tb < 1 || rows < 1) return "need B, Ta, Tb, rows >= 1";
    return std::string();
}

}  // namespace tts
