// Short-time objective intelligibility (STOI, Taal et al. 2011; ESTOI, Jensen and Taal 2016), host side: the frame and segment
// counts, the window and the band table, the groupings of the five launches with their LDS bytes, and the argument checks of
// tts_stoi.  Plain C++ (no HIP, no handle): stoi.hip includes it, and tests/stoi_check.cpp compiles it alone.
//
// A row of n samples at 10 kHz has stoi_frames(n) frames of STOI_W samples, STOI_H apart.  The energy launch gives a lane a
// frame and a workgroup STOI_ENERGY_FRAMES of them; the scan launch gives a row to one workgroup whose lanes own a run of
// stoi_scan_run(frames) consecutive frames each; the envelope launch gives a workgroup STOI_GROUP kept frames, two complex
// double transforms of STOI_NFFT / 2 points in LDS apiece (a real transform of STOI_NFFT points per signal); the segment launch gives a lane a segment and a workgroup
// STOI_SEG_CHUNK of them, over a tile of STOI_SEG_CHUNK + STOI_N - 1 frames of both envelopes; the last launch adds a row's
// segment sums in order.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int STOI_W = 256;                  // samples of a frame
constexpr int STOI_H = 128;                  // samples between two frames
constexpr int STOI_NFFT = 512;               // points of the transform (a frame, zero-padded)
constexpr int STOI_J = 15;                   // one-third octave bands
constexpr int STOI_N = 30;                   // frames of a segment
constexpr int STOI_UTTS = 64;                // rows per launch: their lengths travel by value
constexpr int STOI_ENERGY_FRAMES = 64;       // frames (lanes) of an energy workgroup
constexpr int STOI_SCAN_LANES = 256;         // lanes of the scan's workgroup
constexpr int STOI_SCAN_RUN = 256;           // consecutive frames a lane of the scan owns at most
constexpr int STOI_MAX_FRAMES = STOI_SCAN_LANES * STOI_SCAN_RUN;   // what the scan takes: 65536 frames, 13.9 minutes at 10 kHz
constexpr int STOI_GROUP = 4;                // kept frames of an envelope workgroup
constexpr int STOI_ENV_LANES = 256;          // ... and its lanes
constexpr int STOI_SEG_CHUNK = 64;           // segments (lanes) of a segment workgroup
constexpr size_t STOI_LDS_BUDGET = 48 * 1024;   // bytes of LDS a workgroup may ask for: three workgroups share a compute unit

// (constexpr: the kernels call these too)
constexpr int stoi_frames(int n) { return n < STOI_W ? 0 : (n - STOI_W) / STOI_H + 1; }
constexpr int stoi_segments(int kept) { return kept >= STOI_N ? kept - (STOI_N - 1) : 0; }
constexpr long long stoi_compacted(int kept) { return kept < 1 ? 0 : (long long)(kept - 1) * STOI_H + STOI_W; }
constexpr int stoi_groups(int count, int per) { return count < 1 ? 1 : (count + per - 1) / per; }   // (a launch has one workgroup at least)
constexpr int stoi_scan_run(int frames) { return (frames + STOI_SCAN_LANES - 1) / STOI_SCAN_LANES; }
// the energy workgroup stages the samples of its frames as floats, sample q at q + q / STOI_H: the lanes' walks, STOI_H samples
// apart, fall on different banks
constexpr size_t stoi_energy_floats() { return (size_t)(STOI_ENERGY_FRAMES + 1) * (STOI_H + 1); }
constexpr size_t stoi_energy_lds_bytes() { return sizeof(float) * stoi_energy_floats(); }
// the envelope workgroup: per frame two transforms of STOI_NFFT / 2 complex doubles (8 KB a frame), the twiddles
// exp(-2 pi i k / STOI_NFFT), k < STOI_NFFT / 2, and the window
constexpr size_t stoi_env_lds_bytes() {
    return 2 * sizeof(double) * ((size_t)STOI_GROUP * STOI_NFFT + STOI_NFFT / 2) + sizeof(double) * STOI_W;
}
// the segment workgroup: both envelopes' J bands over the frames of its segments
constexpr int stoi_seg_tile_frames() { return STOI_SEG_CHUNK + STOI_N - 1; }
constexpr size_t stoi_seg_lds_bytes() { return sizeof(double) * 2 * STOI_J * (size_t)stoi_seg_tile_frames(); }

// w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), which is np.hanning(258)[1:-1] -- evaluated in the form numpy takes,
// 0.5 + 0.5 cos(pi (2 i - 255) / 257): near its ends the window is a difference of two numbers near 0.5, and only the same
// form gives the same last bits
inline void stoi_window(double w[STOI_W]) {
    const double pi = 3.141592653589793;
    for (int i = 0; i < STOI_W; ++i) w[i] = 0.5 + 0.5 * std::cos(pi * (double)(2 * i - (STOI_W - 1)) / (double)(STOI_W + 1));
}

// One-third octave bands from 150 Hz at 10 kHz: band k takes the bins [lo, hi) of the 512-point transform, lo and hi the bins
// nearest to 150 * 2 ** ((2 k - 1) / 6) and 150 * 2 ** ((2 k + 1) / 6) Hz (the first of two equally near).
inline void stoi_bands(int32_t edges[STOI_J][2]) {
    const double df = 10000.0 / (double)STOI_NFFT;
    for (int k = 0; k < STOI_J; ++k)
        for (int side = 0; side < 2; ++side) {
            const double f = 150.0 * std::pow(2.0, (double)(2 * k + (side ? 1 : -1)) / 6.0);
            int best = 0;
            double dist = f * f;
            for (int b = 1; b <= STOI_NFFT / 2; ++b) {
                const double d = ((double)b * df - f) * ((double)b * df - f);
                if (d < dist) dist = d, best = b;
            }
            edges[k][side] = best;
        }
}

// The checks of tts_stoi, in the order the header lists them.  An empty string: the call is legal.  *unsupported is set where
// the refusal is a frame count beyond the scan (TTS_ERR_UNSUPPORTED), cleared otherwise (TTS_ERR_INVALID).  The pointers come as
// integers: ref, deg and records are required, index and envelopes may be 0.  n_samples: host lengths or null (all N).
inline std::string stoi_check(uintptr_t ref, uintptr_t deg, uintptr_t records, uintptr_t index, uintptr_t envelopes, int B, int N,
                              const int32_t* n_samples, int extended, bool* unsupported) {
    *unsupported = false;
    if (!ref || !deg || !records) return "a NULL pointer (ref, deg and records are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    const std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N);
    if (!bad.empty()) return bad;
    if (extended != 0 && extended != 1) return "extended = " + std::to_string(extended) + " is not 0 or 1";
    if (((ref | deg | index) & 3) || ((records | envelopes) & 7)) return "ref, deg and kept_index must be 4-byte aligned, records and envelopes 8-byte aligned";
    if (stoi_frames(N) > STOI_MAX_FRAMES) {
        *unsupported = true;
        return std::to_string(stoi_frames(N)) + " frames are more than tts_stoi_max_frames() = " + std::to_string(STOI_MAX_FRAMES);
    }
    return std::string();
}

}  // namespace tts
