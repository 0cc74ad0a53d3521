// Timing marks, host side: how tts_token_times cuts its work -- utterances per launch, how the lanes of a workgroup cover the
// columns of the table, where the directions of the search live -- the weight of an element (host, kernel and
// tests/marks_oracle.py share this one definition) and the argument checks.  Plain C++ (no HIP, no handle): token_times.hip
// includes it, and tests/token_times_check.cpp compiles it alone.
//
// The cut:
//   a launch takes TT_UTTS utterances, whose lengths travel by value; B utterances are 2 * length_chunks(B, TT_UTTS) launches:
//   positions  the row kernel of the attention diagnostics (alignment.hip): pos[s], what `agree` compares the path with
//   search     one workgroup of TT_THREADS lanes per utterance: lane t holds columns t, t + TT_THREADS, ... -- TT_PASSES of them,
//              hence TT_MAX_TOKENS -- two rows of int64 in LDS, one byte of direction per cell
// The directions of a launch whose longest utterance has `longest` steps are longest * Ts bytes per workgroup: in LDS behind the
// two rows where that is at most TT_DIR_LDS_BYTES, else in a workspace of the handle's.
#pragma once
#include "lengths.h"
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int TT_UTTS = 64;        // utterances per launch: their lengths travel by value
constexpr int TT_THREADS = 256;    // lanes of a workgroup
constexpr int TT_PASSES = 4;       // columns of a lane
constexpr int TT_MAX_TOKENS = TT_THREADS * TT_PASSES;   // tts_token_times_max_tokens()
constexpr int TT_MAX_JUMP = 15;    // the largest max_jump: a direction is a nibble's worth
constexpr int TT_LAUNCHES_PER_CHUNK = 2;
constexpr size_t TT_DIR_LDS_BYTES = 32768;   // with the two rows of TT_MAX_TOKENS int64: 48 KiB, under the 64 KiB of a workgroup

constexpr int tt_launches(int B) { return TT_LAUNCHES_PER_CHUNK * ((B + TT_UTTS - 1) / TT_UTTS); }
constexpr size_t tt_rows_bytes(int Ts) { return 2 * (size_t)Ts * sizeof(int64_t); }
constexpr size_t tt_dir_bytes(int longest, int Ts) { return (size_t)longest * (size_t)Ts; }
constexpr bool tt_dir_in_lds(int longest, int Ts) { return tt_dir_bytes(longest, Ts) <= TT_DIR_LDS_BYTES; }
// the dynamic LDS of a launch
constexpr size_t tt_lds_bytes(int longest, int Ts) { return tt_rows_bytes(Ts) + (tt_dir_in_lds(longest, Ts) ? tt_dir_bytes(longest, Ts) : 0); }

// The weight of an element: its own bit pattern where it is greater than 0 (+Inf included), 0 for a NaN, a zero of either sign
// or a negative value.  Bit patterns with the sign set and the NaNs lie above +Inf's as unsigned integers.
constexpr uint32_t tt_weight(uint32_t bits) { return bits <= 0x7f800000u ? bits : 0u; }

// The checks of tts_token_times, in the order the header lists them.  An empty string: the call is legal so far
// (TTS_ERR_INVALID otherwise).  n_sent, n_steps: host lengths or null.
inline std::string token_times_check(bool have_ptrs, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                                     int max_jump) {
    if (!have_ptrs) return "a NULL pointer (alignments, start and stats are required)";
    if (B < 1 || Ts < 1 || n_steps_max < 1) return "need B, Ts, n_steps_max >= 1";
    const std::string bad = lengths_refusal("n_sent", n_sent, B, "Ts", Ts);
    if (!bad.empty()) return bad;
    const std::string worse = lengths_refusal("n_steps", n_steps, B, "n_steps_max", n_steps_max);
    if (!worse.empty()) return worse;
    if (max_jump < 1 || max_jump > TT_MAX_JUMP)
        return "max_jump = " + std::to_string(max_jump) + " is not in 1 .. " + std::to_string(TT_MAX_JUMP);
    return std::string();
}

// ... and what a legal call is still refused for (TTS_ERR_UNSUPPORTED)
inline std::string token_times_unsupported(int Ts) {
    if (Ts > TT_MAX_TOKENS) return "Ts = " + std::to_string(Ts) + " is above the " + std::to_string(TT_MAX_TOKENS) + " tokens of a table";
    return std::string();
}

}  // namespace tts
