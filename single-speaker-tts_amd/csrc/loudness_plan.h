// Loudness after ITU-R BS.1770-4 / EBU R 128, host side: the K-weighting filters of a sampling rate, the cut of an utterance into
// steps, segments and blocks, the recurrence every side runs (host, kernel and tests/loudness_oracle.py share this one
// definition) and the argument checks of tts_loudness, tts_loudness_normalize and tts_set_loudness.  Plain C++ (no HIP, no
// handle): loudness.hip includes it, and tests/loudness_check.cpp compiles it alone.
//
// The cut, a function of the sampling rate alone:
//   s = sr / 10 samples are a 100 ms step; an utterance of n samples has K = n / s steps, and the samples behind them count for
//   nothing.  A block is four steps and starts at every step: J = K - 3 blocks (none for K < 4, and nothing is read then).
//   A step is cut into LOUD_SEGS = 8 segments of c = ceil(s / 8) samples, the last one of s - 7 c (1 .. c) samples; one lane owns
//   one segment.
//   pass 1  runs the cascade over each segment from the zero state and keeps the four state values it ends in, e_i.
//   pass 2  chains them along the utterance, S_0 = 0 and, for row r of the segment's 4 x 4 transition M (loud_transition),
//             S_{i+1}[r] = ((((M[r][0] S_i[0] + M[r][1] S_i[1]) + M[r][2] S_i[2]) + M[r][3] S_i[3]) + e_i[r]
//   pass 3  runs each segment again from S_i and sums y * y in sample order from +0.0.
//   u_k is the sum of the step's 8 segment sums in order, ((((((q_0 + q_1) + q_2) + ...) + q_7); block j has
//   z_j = (((u_j + u_j+1) + u_j+2) + u_j+3) / (4 s).
// Every product, sum and quotient is an individually rounded IEEE double operation.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int LOUD_SR_MIN = 8000, LOUD_SR_MAX = 192000;
constexpr int LOUD_SEGS = 8;                             // segments of a step
constexpr int LOUD_UTTS = 64;                            // utterances per launch: their lengths travel by value
constexpr double LOUD_Z_ABS = 1.1724653045822981e-07;    // the absolute gate, 10 ** ((-70 + 0.691) / 10), in the mean-square domain
constexpr double LOUD_REL = 0.1;                         // the relative gate, -10 dB

// (constexpr: the kernels call these too)
constexpr int loud_step(int sr) { return sr / 10; }
constexpr int loud_segment(int sr) { return (loud_step(sr) + LOUD_SEGS - 1) / LOUD_SEGS; }
constexpr int loud_last_segment(int sr) { return loud_step(sr) - (LOUD_SEGS - 1) * loud_segment(sr); }
constexpr int loud_segment_len(int sr, int q) { return q < LOUD_SEGS - 1 ? loud_segment(sr) : loud_last_segment(sr); }
constexpr int loud_steps(int n, int sr) { return n / loud_step(sr); }
constexpr int loud_blocks(int n, int sr) { return loud_steps(n, sr) >= 4 ? loud_steps(n, sr) - 3 : 0; }
// the steps that are read at all: those of an utterance with a block
constexpr int loud_steps_read(int n, int sr) { return loud_blocks(n, sr) ? loud_steps(n, sr) : 0; }

// b0 b1 b2 a1 a2 of the shelf, then of the high-pass
struct LoudFilter {
    double k[10];
};

// The design: the bilinear transform of the analogue prototypes that reproduce the standard's 48 kHz tables.
inline LoudFilter loud_filter(int sr) {
    LoudFilter f;
    const double pi = 3.141592653589793;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)sr), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        f.k[0] = (Vh + Vb * K / Q + K * K) / a0;
        f.k[1] = 2.0 * (K * K - Vh) / a0;
        f.k[2] = (Vh - Vb * K / Q + K * K) / a0;
        f.k[3] = 2.0 * (K * K - 1.0) / a0;
        f.k[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)sr);
        const double a0 = 1.0 + K / Q + K * K;
        f.k[5] = 1.0;
        f.k[6] = -2.0;
        f.k[7] = 1.0;
        f.k[8] = 2.0 * (K * K - 1.0) / a0;
        f.k[9] = (1.0 - K / Q + K * K) / a0;
    }
    return f;
}

// One sample through the cascade, direct form II transposed; st: z1, z2 of the shelf, then of the high-pass.  Returns y.
constexpr double loud_sample(const double* k, double* st, double x) {
    const double y1 = k[0] * x + st[0];
    st[0] = (k[1] * x - k[3] * y1) + st[1];
    st[1] = k[2] * x - k[4] * y1;
    const double y = k[5] * y1 + st[2];
    st[2] = (k[6] * y1 - k[8] * y) + st[3];
    st[3] = k[7] * y1 - k[9] * y;
    return y;
}

// The transition of `len` samples, row-major M[r][j]: column j is the state the recurrence ends in from the unit state j on
// zero input.
inline void loud_transition(const double* k, int len, double* M) {
    for (int j = 0; j < 4; ++j) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        st[j] = 1.0;
        for (int i = 0; i < len; ++i) loud_sample(k, st, 0.0);
        for (int r = 0; r < 4; ++r) M[4 * r + j] = st[r];
    }
}

// One link of the chain of pass 2: S <- M S + e.
constexpr void loud_chain(const double* M, const double* e, double* S) {
    double n[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < 4; ++r) n[r] = (((M[4 * r] * S[0] + M[4 * r + 1] * S[1]) + M[4 * r + 2] * S[2]) + M[4 * r + 3] * S[3]) + e[r];
    for (int r = 0; r < 4; ++r) S[r] = n[r];
}

// doubles of workspace an utterance of N samples asks for: states [segments][4], segment sums, step sums, block means
inline size_t loud_ws_doubles(int N, int sr) {
    const size_t K = (size_t)loud_steps_read(N, sr);
    return K * LOUD_SEGS * 5 + 2 * K + 1;
}

// The checks of tts_loudness (normalize = false: target_lufs and max_peak are not looked at), tts_loudness_normalize and -- with
// have_ptrs = true, B = N = 1 and no lengths -- tts_set_loudness, in the order the header lists them.  An empty string: the call
// is legal.  *unsupported is set where the refusal is a sampling rate outside the limits (TTS_ERR_UNSUPPORTED), cleared otherwise
// (TTS_ERR_INVALID).  n_samples: host lengths or null (all N).
inline std::string loudness_check(bool have_ptrs, int B, int N, const int32_t* n_samples, int sampling_rate, bool normalize, double target_lufs,
                                  double max_peak, bool* unsupported) {
    *unsupported = false;
    if (!have_ptrs) return normalize ? "a NULL pointer (wav is required)" : "a NULL pointer (wav and mean_square are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    const std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N);
    if (!bad.empty()) return bad;
    if (normalize) {
        if (!std::isfinite(target_lufs)) return "the target must be a finite number of LUFS";
        if (!(std::isfinite(max_peak) && max_peak > 0.0)) return "max_peak must be finite and positive";
    }
    if (sampling_rate < LOUD_SR_MIN || sampling_rate > LOUD_SR_MAX) {
        *unsupported = true;
        return "the sampling rate " + std::to_string(sampling_rate) + " is not in " + std::to_string(LOUD_SR_MIN) + " .. " + std::to_string(LOUD_SR_MAX);
    }
    return std::string();
}

}  // namespace tts
