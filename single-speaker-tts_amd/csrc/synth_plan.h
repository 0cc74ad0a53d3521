// One tts_synthesize call, host side: the frame counts its settings -- end-of-speech stopping, speaking rate, pitch -- leave it
// (`synth_shape`, with the refusals) and the per-utterance lengths that follow from the detected ones (`synth_lengths`).
// Plain C++ (no HIP, no handle): the pipeline includes it, and tests/synth_plan_check.cpp compiles it alone.  DESIGN.md has
// the table of these lengths per setting.
#pragma once
#include <algorithm>
#include <vector>
#include "resample_plan.h"
#include "stretch_plan.h"

namespace tts {

// the shortest utterance Griffin-Lim takes: the smallest n with hop (n - 1) > n_fft / 2
inline int speech_min_frames(int n_fft, int hop) { return (n_fft / 2) / hop + 2; }

// The call's shape, as the handle's settings stood when it was made.  Rate 1.0 and pitch 0: stretch = pitch = false,
// Tw = Tg = T, and nothing of the call changes.
struct SynthShape {
    bool stretch = false;   // Griffin-Lim reconstructs from the time-stretch of the call's magnitudes
    bool pitch = false;     // ... writes its samples un-normalised to a buffer of its own, and the resampler takes them by rho
    double rate = 1.0;      // what the magnitudes are stretched by: the speaking rate s, with a pitch s * rho
    double rate_s = 1.0;    // the speaking rate
    double rho = 1.0;       // exp2(-octaves): the resampling ratio
    int Tw = 0;             // frames of the waveform rows, hop (Tw - 1) samples: stretched_frames(T, s) -- the call without pitch
    int Tg = 0;             // frames Griffin-Lim reconstructs from: stretched_frames(T, rate)
    int min_frames = 1;
};

// A refusal comes back as a non-empty string (TTS_ERR_INVALID, every one of them), in the order a call meets them.
inline std::string synth_shape(int T, int n_fft, int hop, double speaking_rate, double pitch_octaves, bool end_of_speech, SynthShape* out) {
    SynthShape& s = *out;
    s = SynthShape();
    s.Tw = s.Tg = T;
    s.min_frames = hop >= 1 ? speech_min_frames(n_fft, hop) : 1;   // (such a hop is refused here or by Griffin-Lim's own checks)
    const std::string least = std::to_string(s.min_frames) + " (hop (n - 1) > n_fft / 2)";
    if (speaking_rate != 1.0 || pitch_octaves != 0.0) {
        if (hop < 1) return "hop_length >= 1";
        s.stretch = true;
        s.rate = s.rate_s = speaking_rate;
        if (s.rate_s != 1.0) s.Tw = (int)stretched_frames(T, s.rate_s);
        if (pitch_octaves != 0.0) {
            s.pitch = true;
            s.rho = std::exp2(-pitch_octaves);
            s.rate = s.rate_s * s.rho;
            if (!stretch_rate_ok(s.rate))
                return "the speaking rate times 2 ** -octaves of the pitch is " + std::to_string(s.rate) + ", outside [0.25, 4]";
            // (the rows of a shifted call are those of the call without pitch, which this refusal is of: Tw = T at rate 1.0)
            if (s.Tw < s.min_frames)
                return "with a pitch the call's rows hold " + std::to_string(s.Tw) + " frames" + (s.rate_s != 1.0 ? " at this speaking rate" : "") +
                       ", the call without pitch needs at least " + least;
        }
        s.Tg = (int)stretched_frames(T, s.rate);
        if (s.Tg < s.min_frames)
            return std::string("the speaking rate") + (s.pitch ? " and the pitch leave " : " leaves ") + std::to_string(s.Tg) +
                   " frames, Griffin-Lim needs at least " + least;
    }
    if (end_of_speech && T < s.min_frames) return "end-of-speech stopping needs at least " + std::to_string(s.min_frames) + " frames (hop (n - 1) > n_fft / 2)";
    return std::string();
}

// The per-utterance lengths of a call, in frames and samples.
struct SynthLengths {
    std::vector<int32_t> reported;    // what the call reports (tts_synth_frames): the lengths of the call without pitch
    std::vector<int32_t> gl;          // what Griffin-Lim runs on
    std::vector<int32_t> n_samples;   // the resampler's input, hop (gl - 1); empty without a pitch or without detected lengths
    std::vector<int32_t> keep;        // ... and where its rows end, hop (reported - 1): with the un-shifted call's utterances
    bool ragged = false;              // sum(gl) != B Tg: Griffin-Lim is given `gl`
    int T_model = 0;                  // the mean of `gl`, rounded up (gl_wide_from's model counts frames)
};

// detected: the B lengths of the end-of-speech detection, each in [min_frames, T], or null -- all T.  An utterance of n frames
// has min(T_r, max(min_frames, stretched_frames(n, r))) at rate r in rows of T_r; at rate 1.0 its length is n untouched.
inline void synth_lengths(const SynthShape& s, int T, int hop, int B, const int32_t* detected, SynthLengths* out) {
    SynthLengths& L = *out;
    const auto at_rate = [&s](int n, double r, int T_r) {
        return (int32_t)std::min<long long>(T_r, std::max<long long>(s.min_frames, stretched_frames(n, r)));
    };
    L.reported.resize((size_t)B);
    L.gl.resize((size_t)B);
    long long sum = 0;
    for (int b = 0; b < B; ++b) {
        const int n = detected ? detected[b] : T;
        L.gl[b] = s.stretch ? at_rate(n, s.rate, s.Tg) : n;
        // (with a pitch Griffin-Lim runs on the lengths at rate s rho, and the call reports those at rate s: the un-shifted call's)
        L.reported[b] = !s.pitch ? L.gl[b] : s.rate_s != 1.0 ? at_rate(n, s.rate_s, s.Tw) : n;
        sum += L.gl[b];
    }
    L.ragged = sum != (long long)B * s.Tg;
    L.T_model = (int)((sum + B - 1) / B);
    const size_t shifted = s.pitch && detected ? (size_t)B : 0;
    L.n_samples.resize(shifted);
    L.keep.resize(shifted);
    for (size_t b = 0; b < shifted; ++b) {
        L.n_samples[b] = hop * (L.gl[b] - 1);
        L.keep[b] = hop * (L.reported[b] - 1);
    }
}

}  // namespace tts
