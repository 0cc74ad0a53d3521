// Attention diagnostics, host side: how tts_alignment_stats cuts its work -- utterances per launch, rows per workgroup, how a
// wave covers a row of any length and address in 16-byte loads -- the order an argmax is decided in (host, kernel and
// tests/alignment_oracle.py share this one definition) and the argument checks.  Plain C++ (no HIP, no handle): alignment.hip
// includes it, and tests/alignment_check.cpp compiles it alone.
//
// The cut:
//   a launch takes ALIGN_UTTS utterances, whose lengths travel by value; B utterances are 2 * length_chunks(B, ALIGN_UTTS) launches
//   rows     one wave per row (s, b), ALIGN_ROWS waves to a workgroup: grid (ceil(steps / ALIGN_ROWS), utterances)
//   walk     one wave per utterance
// A row of Ts floats whose first element lies `mis` floats behind a 16-byte boundary is read as head = min(Ts, (4 - mis) % 4)
// single floats, (Ts - head) / 4 aligned float4s and the rest as single floats again: every element exactly once, none outside.
#pragma once
#include "lengths.h"
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int ALIGN_UTTS = 64;   // utterances per launch: their lengths travel by value
constexpr int ALIGN_ROWS = 4;    // rows (waves) of a workgroup of the row kernel
constexpr int ALIGN_LAUNCHES_PER_CHUNK = 2;

constexpr int align_launches(int B) { return ALIGN_LAUNCHES_PER_CHUNK * ((B + ALIGN_UTTS - 1) / ALIGN_UTTS); }
constexpr int align_row_blocks(int steps) { return (steps + ALIGN_ROWS - 1) / ALIGN_ROWS; }

// how a wave covers a row (constexpr: the kernel calls these too)
struct AlignCover {
    int head, vecs, tail;   // single floats, aligned float4s behind them, single floats behind those
};
constexpr AlignCover align_cover(int mis, int Ts) {
    const int want = (4 - (mis & 3)) & 3;
    const int head = want < Ts ? want : Ts;
    const int vecs = (Ts - head) / 4;
    return AlignCover{head, vecs, Ts - head - 4 * vecs};
}

// The order of an argmax: a candidate is a 64-bit key, and the LARGEST key wins.  The high word orders the values as numpy's
// argmax does -- NaN above everything, then +Inf down to -Inf, -0 equal to +0 -- and the low word the indices, the lower the
// larger: the lowest index of the maximum, or the first NaN.  A maximum over keys is free of any order of evaluation.  No key is 0.
constexpr uint32_t align_value_key(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;     // NaN
    if ((bits & 0x7fffffffu) == 0u) return 0x80000000u;             // +0 and -0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
constexpr uint64_t align_key(uint32_t bits, uint32_t index) {
    return ((uint64_t)align_value_key(bits) << 32) | (uint64_t)(0xffffffffu - index);
}
constexpr int align_key_index(uint64_t key) { return (int)(0xffffffffu - (uint32_t)(key & 0xffffffffu)); }

// The checks of tts_alignment_stats, in the order the header lists them.  An empty string: the call is legal (TTS_ERR_INVALID
// otherwise).  n_sent, n_steps: host lengths or null.
inline std::string alignment_check(bool have_ptrs, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps) {
    if (!have_ptrs) return "a NULL pointer (alignments and stats are required)";
    if (B < 1 || Ts < 1 || n_steps_max < 1) return "need B, Ts, n_steps_max >= 1";
    const std::string bad = lengths_refusal("n_sent", n_sent, B, "Ts", Ts);
    if (!bad.empty()) return bad;
    return lengths_refusal("n_steps", n_steps, B, "n_steps_max", n_steps_max);
}

// ... and of tts_text_lengths
inline std::string text_lengths_check(bool have_ptrs, int B, int Ts) {
    if (!have_ptrs) return "a NULL pointer (ids and n_sent are required)";
    if (B < 1 || Ts < 1) return "need B, Ts >= 1";
    return std::string();
}

}  // namespace tts
