// Prosody, host side: the checks of a warp's segment list, the output frames of every segment and row, and how the list is cut
// into launches and tiles (host, kernel and tests/warp_oracle.py share this one definition).  Plain C++ (no HIP, no handle):
// warp.hip includes it, and tests/warp_check.cpp compiles it alone.
//
// The layout of a row: segment s starts at output frame o[s]; o of a row's first segment is 0, o[s+1] = o[s] + count[s], and the
// row holds n_out = o[last] + count[last] frames.  count of a speech segment is ceil(frames * 65536 / step) -- the output frames j
// whose source position j * step / 65536 lies inside the segment --, of a pause its `pause`.
//
// The cut: every output frame of a row is OWNED by exactly one segment -- segment s owns [o[s], o[s+1]), a row's last segment
// [o[s], T_out): its own frames and behind them the zeros of the row's rest.  A workgroup takes WARP_TILE consecutive frames of what
// one segment owns, in WARP_BINS bins; segments.h has the list's order, the launches and the numbering of their tiles.  The launches
// of a call write disjoint ranges that cover out[B][F][T_out]: every element once.
#pragma once
#include "segments.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sstts_hip.h"

namespace tts {

constexpr int WARP_SEGMENTS = SEGMENTS_PER_LAUNCH, WARP_MAX_SEGMENTS = MAX_SEGMENTS;
constexpr int WARP_THREADS = 256;
constexpr int WARP_TILE = 64;                // output frames of a workgroup: one wave along the frames, a bin per wave and round
constexpr int WARP_BINS = 32;                // bins of a workgroup: WARP_BINS / (WARP_THREADS / WARP_TILE) rounds
constexpr uint32_t WARP_STEP_MIN = 16384, WARP_STEP_MAX = 262144;   // the rates 0.25 .. 4 of stretch_rate_ok, times 65536
constexpr float WARP_GAIN_MAX = 16.f;
constexpr int WARP_MAX_T_OUT = 1 << 30;

constexpr int warp_launches(int S) { return segment_launches(S); }
constexpr int64_t warp_tiles(int64_t span) { return (span + WARP_TILE - 1) / WARP_TILE; }

// output frames of a speech segment: the j >= 0 with j * step < frames * 65536 (exact in int64: frames < 2^31)
constexpr int64_t warp_count(int32_t frames, uint32_t step) { return (((int64_t)frames << 16) + (int64_t)step - 1) / (int64_t)step; }

// What the kernel knows of a segment: the row, where its source starts, the output frames it owns ([o, o + span), of which the
// first `count` are blended and the rest is zero), the frames of its row that may be read, and its first tile in the launch.
struct WarpEntry {
    int32_t row, first, o, count, span, n, tile0;
    uint32_t step;
    float gain;
};
using WarpChunk = SegmentChunk<WarpEntry>;
constexpr WarpEntry WARP_NO_ENTRY{0, 0, 0, 0, 0, 0, 0, 0, 0.f};   // what pads a launch's chunk

// The checks of tts_warp_plan and tts_warp_magnitudes on the list, in the order the header lists them, and the lengths.  An
// empty string: the list is legal (TTS_ERR_INVALID otherwise).  n_out [B], and count [S] where it is given, are filled.
inline std::string warp_plan(const tts_warp_segment_t* seg, int S, int B, int T, const int32_t* n_frames, int64_t* n_out, int64_t* count = nullptr) {
    if (!seg || !n_out) return "a NULL pointer (segments and n_out are required)";
    if (B < 1 || T < 1 || S < 1) return "need B, T, S >= 1";
    const std::string bad = segment_rows_refusal(seg, S, B, "tts_warp_max_segments()", "n_frames", n_frames, "T", T);
    if (!bad.empty()) return bad;
    int64_t o = 0;
    for (int s = 0; s < S; ++s) {
        const tts_warp_segment_t& q = seg[s];
        const std::string name = "segment " + std::to_string(s);
        if (q.frames < 0 || q.pause < 0) return name + " has a negative length (frames " + std::to_string(q.frames) + ", pause " + std::to_string(q.pause) + ")";
        if (q.frames > 0 && q.pause > 0)
            return name + " is both speech (" + std::to_string(q.frames) + " frames) and a pause (" + std::to_string(q.pause) + " frames)";
        if (q.frames == 0 && q.pause == 0) return name + " is neither speech nor a pause (frames and pause are 0)";
        int64_t c = q.pause;
        if (q.frames > 0) {
            const int n = n_frames ? n_frames[q.row] : T;
            if (q.first < 0 || (int64_t)q.first + q.frames > (int64_t)n)
                return name + " reads frames " + std::to_string(q.first) + " .. " + std::to_string((int64_t)q.first + q.frames - 1) + " of row " +
                       std::to_string(q.row) + ", which has 0 .. " + std::to_string(n - 1);
            if (q.step < WARP_STEP_MIN || q.step > WARP_STEP_MAX)
                return name + " has step " + std::to_string(q.step) + ", which is not in " + std::to_string(WARP_STEP_MIN) + " .. " + std::to_string(WARP_STEP_MAX);
            if (!(q.gain >= 0.f && q.gain <= WARP_GAIN_MAX))   // (a NaN fails both comparisons)
                return name + " has a gain that is not finite or lies outside 0 .. 16";
            c = warp_count(q.frames, q.step);
        }
        if (count) count[s] = c;
        o += c;
        if (s + 1 == S || seg[s + 1].row != q.row) {
            n_out[q.row] = o;
            o = 0;
        }
    }
    return std::string();
}

// ... and of tts_warp_magnitudes' own arguments behind a legal list
inline std::string warp_room(const int64_t* n_out, int B, int T_out) { return segment_room("T_out", n_out, B, T_out, WARP_MAX_T_OUT); }

// The entries of a legal list (count from warp_plan, every n_out <= T_out) with every launch's own tile numbering: entry s is
// segment s, and tiles[l] the workgroups along the frames of launch l.
inline void warp_entries(const tts_warp_segment_t* seg, int S, int T, const int32_t* n_frames, int T_out, const int64_t* count, std::vector<WarpEntry>& e,
                         std::vector<int64_t>& tiles) {
    e.assign((size_t)S, WARP_NO_ENTRY);
    tiles.assign((size_t)segment_launches(S), 0);
    int64_t o = 0;
    for (int s = 0; s < S; ++s) {
        const tts_warp_segment_t& q = seg[s];
        const bool last = s + 1 == S || seg[s + 1].row != q.row;
        const bool speech = q.frames > 0;
        WarpEntry& w = e[(size_t)s];
        w.row = q.row;
        w.first = speech ? q.first : 0;
        w.o = (int32_t)o;
        w.count = speech ? (int32_t)count[s] : 0;
        w.span = (int32_t)(last ? (int64_t)T_out - o : count[s]);
        w.n = n_frames ? n_frames[q.row] : T;
        w.step = speech ? q.step : 65536u;
        w.gain = speech ? q.gain : 0.f;
        w.tile0 = segment_take_tiles(tiles, s, warp_tiles(w.span));
        o = last ? 0 : o + count[s];
    }
}

}  // namespace tts
