// Estimated initial phases, host side: how the frames of an utterance are cut into chunks and the argument checks of the
// estimate's entry points.  Plain C++ (no HIP, no handle): phase_init.hip includes it, and tests/phase_check.cpp compiles it alone.
#pragma once
#include "lengths.h"
#include <cstdint>
#include <string>

namespace tts {

constexpr int PE_CHUNK = 32;          // frames a workgroup takes one after the other (phase_init.hip)
constexpr int PE_UTTS = 64;           // utterances per launch: their lengths travel by value
constexpr int PE_MIN_NFFT = 256, PE_MAX_NFFT = 4096;   // what the audio surface takes (glg_supports)
constexpr int PE_MAX_FRAMES = 1 << 22;                 // chunk counts and tile grids stay far inside an int

// chunks of an utterance of n frames; 0 for n < 1
inline int pe_chunks(int n) { return n < 1 ? 0 : (n + PE_CHUNK - 1) / PE_CHUNK; }

inline bool pe_nfft_ok(int n_fft) { return n_fft >= PE_MIN_NFFT && n_fft <= PE_MAX_NFFT && (n_fft & (n_fft - 1)) == 0; }

// The checks of tts_phase_estimate / tts_phase_estimate_rows, in the order the header lists them; an empty string: the call is
// legal.  n_frames: host lengths or null (all T).  have_ptrs: the data pointers are not NULL.  row_stride: floats between two
// rows of the time-major layout (1 + n_fft / 2 for the public layout, which has no stride).
inline std::string phase_check(bool have_ptrs, int B, int T, int row_stride, const int32_t* n_frames, int n_fft, int hop_length) {
    if (!have_ptrs) return "a NULL pointer";
    if (!pe_nfft_ok(n_fft)) return "n_fft must be a power of two between 256 and 4096";
    if (hop_length < 1 || hop_length > n_fft) return "need 1 <= hop_length <= n_fft";
    if (B < 1 || T < 1) return "need B, T >= 1";
    if (T > PE_MAX_FRAMES) return "T is larger than " + std::to_string(PE_MAX_FRAMES);
    if (row_stride < 1 + n_fft / 2) return "row_stride < 1 + n_fft / 2";
    return lengths_refusal("n_frames", n_frames, B, "T", T);
}

}  // namespace tts
