// Per-word pitch, host side: the checks of a segment-wise resampling's list, the output samples of every segment and row, the
// ratios whose tables a call needs, and how the list is cut into launches and tiles (host, kernel and
// tests/resample_segments_oracle.py share this one definition).  Plain C++ (no HIP, no handle): resample_segments.hip includes it,
// and tests/resample_segments_check.cpp compiles it alone.
//
// The layout of a row: segment s starts at output sample o[s]; o of a row's first segment is 0, o[s+1] = o[s] + count[s], and the
// row holds n_out = o[last] + count[last] samples.  count of a segment at ratio 1.0 exactly -- a COPY -- is its `samples`, of any
// other resampled_valid(samples, ratio) = (long long)(samples * ratio), resampy's; a segment may produce no sample.
//
// The cut: every output sample of a row is OWNED by exactly one segment -- segment s owns [o[s], o[s+1]), a row's last segment
// [o[s], N_out): its own samples and behind them the zeros of the row's rest.  A workgroup takes RSEG_TILE consecutive samples of
// what one segment owns, and a segment that owns nothing has no tile; segments.h has the list's order, the launches and the
// numbering of their tiles.  The launches of a call write disjoint ranges that cover out[B][N_out]: every element once.
#pragma once
#include "segments.h"
#include "resample_plan.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sstts_hip.h"

namespace tts {

constexpr int RSEG_SEGMENTS = SEGMENTS_PER_LAUNCH, RSEG_MAX_SEGMENTS = MAX_SEGMENTS;
constexpr int RSEG_MAX_RATIOS = 16;        // distinct ratios below 1 per call: each has a table of its own (0.5 MiB)
constexpr int RSEG_TILE = 256;             // output samples of a workgroup, one per thread (resample.hip's RS_TILE)
constexpr int RSEG_MAX_N_OUT = 1 << 30;

constexpr int rseg_launches(int S) { return segment_launches(S); }
constexpr int64_t rseg_tiles(int64_t span) { return (span + RSEG_TILE - 1) / RSEG_TILE; }

inline bool rseg_is_copy(double ratio) { return ratio == 1.0; }
inline int64_t rseg_count(int32_t samples, double ratio) { return rseg_is_copy(ratio) ? (int64_t)samples : (int64_t)resampled_valid(samples, ratio); }

// What the kernel knows of a segment: the row, where its source starts, the output samples it owns ([o, o + span), of which the
// first `count` are copied or resampled and the rest is zero), the samples of its row that may be read, its first tile in the
// launch, the call's table it walks (-1: a copy; 0: the one the ratios above 1 share) and its ratio's inc and scale.
struct RsegEntry {
    int32_t row, first, o, count, span, n, tile0, tab;
    double inc, scale;
};
using RsegChunk = SegmentChunk<RsegEntry>;
constexpr RsegEntry RSEG_NO_ENTRY{0, 0, 0, 0, 0, 0, 0, -1, 1.0, 1.0};   // a copy of nothing: what pads a launch's chunk

// The checks of tts_resample_segments_plan and tts_resample_segments on the list, in the order the header lists them, and the
// lengths.  An empty string: the list is legal (TTS_ERR_INVALID otherwise).  n_out [B], and count [S] where it is given, are filled.
inline std::string resample_segments_plan(const tts_resample_segment_t* seg, int S, int B, int n, const int32_t* n_samples, int64_t* n_out,
                                          int64_t* count = nullptr) {
    if (!seg || !n_out) return "a NULL pointer (segments and n_out are required)";
    if (B < 1 || n < 1 || S < 1) return "need B, n, S >= 1";
    const std::string bad = segment_rows_refusal(seg, S, B, "tts_resample_segments_max()", "n_samples", n_samples, "n", n);
    if (!bad.empty()) return bad;
    int64_t o = 0;
    uint64_t below[RSEG_MAX_RATIOS];
    int n_below = 0, extra_at = -1;   // extra_at: the segment that brings one ratio too many (the later segments are still checked)
    for (int s = 0; s < S; ++s) {
        const tts_resample_segment_t& q = seg[s];
        const std::string name = "segment " + std::to_string(s);
        const int rows = n_samples ? n_samples[q.row] : n;
        if (q.samples < 1) return name + " has " + std::to_string(q.samples) + " samples: at least 1 is needed";
        if (q.first < 0 || (int64_t)q.first + q.samples > (int64_t)rows)
            return name + " reads samples " + std::to_string(q.first) + " .. " + std::to_string((int64_t)q.first + q.samples - 1) + " of row " +
                   std::to_string(q.row) + ", which has 0 .. " + std::to_string(rows - 1);
        if (!resample_ratio_ok(q.ratio)) return name + " has a ratio that is not finite or lies outside [0.25, 4]";
        if (q.reserved != 0) return name + " has reserved = " + std::to_string(q.reserved) + ", which must be 0";
        if (q.ratio < 1.0) {
            uint64_t key = 0;
            std::memcpy(&key, &q.ratio, sizeof(key));
            int k = 0;
            while (k < n_below && below[k] != key) ++k;
            if (k == n_below) {
                if (n_below < RSEG_MAX_RATIOS) below[n_below++] = key;
                else if (extra_at < 0) extra_at = s;
            }
        }
        const int64_t c = rseg_count(q.samples, q.ratio);
        if (count) count[s] = c;
        o += c;
        if (s + 1 == S || seg[s + 1].row != q.row) {
            n_out[q.row] = o;
            o = 0;
        }
    }
    if (extra_at >= 0)
        return "segment " + std::to_string(extra_at) + " brings distinct ratio below 1 number " + std::to_string(RSEG_MAX_RATIOS + 1) +
               ": a call takes tts_resample_segments_max_ratios() = " + std::to_string(RSEG_MAX_RATIOS);
    return std::string();
}

// ... and of tts_resample_segments' own arguments behind a legal list
inline std::string resample_segments_room(const int64_t* n_out, int B, int N_out) { return segment_room("N_out", n_out, B, N_out, RSEG_MAX_N_OUT); }

// The distinct ratios below 1 of a legal list, in the order they first appear (at most RSEG_MAX_RATIOS): table k + 1 of the call
// is below[k]'s.  *above: some segment has a ratio above 1 -- table 0, the one all of them share.
inline void resample_segments_ratios(const tts_resample_segment_t* seg, int S, std::vector<double>& below, bool* above) {
    below.clear();
    *above = false;
    for (int s = 0; s < S; ++s) {
        const double r = seg[s].ratio;
        if (r > 1.0) *above = true;
        if (r < 1.0) {
            size_t k = 0;
            while (k < below.size() && std::memcmp(&below[k], &r, sizeof(r)) != 0) ++k;
            if (k == below.size()) below.push_back(r);
        }
    }
}

// the samples a workgroup of a segment at these constants stages, at most: the windows of RSEG_TILE outputs (resample_span_max)
inline int rseg_span_max(const ResampleConsts& c) { return (int)((double)(RSEG_TILE - 1) * c.inc) + 2 + 2 * c.taps_max; }

// The entries of a legal list (count from resample_segments_plan, every n_out <= N_out, below from resample_segments_ratios) with
// every launch's own tile numbering: entry s is segment s, tiles[l] the workgroups of launch l and lds[l] the floats the largest
// of its resampled segments stages (0: copies alone).
inline void resample_segments_entries(const tts_resample_segment_t* seg, int S, int n, const int32_t* n_samples, int N_out, const int64_t* count,
                                      const std::vector<double>& below, std::vector<RsegEntry>& e, std::vector<int64_t>& tiles, std::vector<int>& lds) {
    e.assign((size_t)S, RSEG_NO_ENTRY);
    tiles.assign((size_t)segment_launches(S), 0);
    lds.assign((size_t)rseg_launches(S), 0);
    int64_t o = 0;
    for (int s = 0; s < S; ++s) {
        const tts_resample_segment_t& q = seg[s];
        const bool last = s + 1 == S || seg[s + 1].row != q.row;
        RsegEntry& w = e[(size_t)s];
        w.row = q.row;
        w.first = q.first;
        w.o = (int32_t)o;
        w.count = (int32_t)count[s];
        w.span = (int32_t)(last ? (int64_t)N_out - o : count[s]);
        w.n = n_samples ? n_samples[q.row] : n;
        if (!rseg_is_copy(q.ratio)) {
            const ResampleConsts c = resample_consts(q.ratio);
            w.inc = c.inc;
            w.scale = c.scale;
            w.tab = 0;
            for (size_t k = 0; k < below.size(); ++k)
                if (std::memcmp(&below[k], &q.ratio, sizeof(double)) == 0) w.tab = (int32_t)k + 1;
            int& most = lds[(size_t)(s / RSEG_SEGMENTS)];
            if (w.count > 0 && rseg_span_max(c) > most) most = rseg_span_max(c);
        }
        w.tile0 = segment_take_tiles(tiles, s, rseg_tiles(w.span));
        o = last ? 0 : o + count[s];
    }
}

}  // namespace tts
