// Segment lists, host and kernel side: what every stage that takes a list of segments shares (the warp, the segment-wise resampler
// and the shift) -- the order of a list's rows and its refusals, how a list is cut into launches, how a launch's tiles are numbered
// and how a workgroup finds its segment.  Plain C++ (no handle; HIP only for segment_find's qualifiers): the *_plan.h headers of
// these stages include it, and tests/segments_check.cpp compiles it alone.
//
// The list: S <= MAX_SEGMENTS records whose first field is `int32_t row`.  The rows start at 0, never decrease, skip none and end at
// B - 1: every row of the batch has at least one segment, and a row's segments are consecutive.
//
// The cut: a launch takes SEGMENTS_PER_LAUNCH consecutive segments, whose entries -- what the kernel knows of a segment, with a
// field `int32_t tile0` -- travel by value (SegmentChunk): nothing is uploaded and nothing synchronised.  The tiles of a launch are
// numbered segment after segment: entry s owns the tiles [tile0, tile0 + its tiles) of launch s / SEGMENTS_PER_LAUNCH, none where
// it owns no tile at all, and workgroup blockIdx.x finds its segment with segment_find.  What a tile is belongs to the stage.
#pragma once
#include "lengths.h"
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace tts {

constexpr int SEGMENTS_PER_LAUNCH = 64;   // segments per launch: their entries travel by value
constexpr int MAX_SEGMENTS = 4096;        // segments per call (64 launches)

constexpr int segment_launches(int S) { return (S + SEGMENTS_PER_LAUNCH - 1) / SEGMENTS_PER_LAUNCH; }

template <class Entry>
struct SegmentChunk {
    Entry e[SEGMENTS_PER_LAUNCH];
};

// The entry that owns tile `tile` of a launch of n_seg >= 1 entries: the last one whose first tile is not behind it (an entry
// without tiles shares its tile0 with its successor, which is the later one).  Workgroup-uniform in a kernel: six scalar steps.
template <class Entry>
inline
#ifdef __HIPCC__
    __host__ __device__
#endif
    int
    segment_find(const Entry* e, int n_seg, int tile) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (e[m].tile0 <= tile) lo = m;
        else hi = m - 1;
    }
    return lo;
}

// The checks of a plan that every stage makes alike, behind its own leading ones (the NULL pointers, need ... >= 1) and in front of
// its own per-segment ones: the counts, the lengths `len` [B] (null: all `hi`) and the order of the rows.  max_name: the stage's
// tts_*_max...() of the public header.  An empty string: legal.
template <class Seg>
inline std::string segment_rows_refusal(const Seg* seg, int S, int B, const char* max_name, const char* len_name, const int32_t* len, const char* bound,
                                        int hi) {
    if (S > MAX_SEGMENTS) return std::to_string(S) + " segments are more than " + max_name + " = " + std::to_string(MAX_SEGMENTS);
    if (B > S) return std::to_string(B) + " rows of " + std::to_string(S) + " segments: no row is without a segment";
    const std::string bad = lengths_refusal(len_name, len, B, bound, hi);
    if (!bad.empty()) return bad;
    if (seg[0].row != 0) return "row of segment 0 is " + std::to_string(seg[0].row) + ": the rows start at 0";
    for (int s = 1; s < S; ++s)
        if (seg[s].row != seg[s - 1].row && seg[s].row != seg[s - 1].row + 1)
            return "row of segment " + std::to_string(s) + " is " + std::to_string(seg[s].row) + " and follows " + std::to_string(seg[s - 1].row) +
                   ": the rows are non-decreasing and none is without a segment";
    if (seg[S - 1].row != B - 1)
        return "row of segment " + std::to_string(S - 1) + " is " + std::to_string(seg[S - 1].row) + ": the last row is B - 1 = " + std::to_string(B - 1);
    return std::string();
}

// ... and of a call's output width `len` (named `name`) behind a legal list whose rows hold n_out [B]: no row is longer, and `len`
// is at most max = 2^30 (a launch's SEGMENTS_PER_LAUNCH segments then own fewer than 2^31 tiles, which is what a launch takes)
inline std::string segment_room(const char* name, const int64_t* n_out, int B, int len, int max) {
    for (int b = 0; b < B; ++b)
        if (n_out[b] > (int64_t)len)
            return std::string(name) + " = " + std::to_string(len) + " is below n_out[" + std::to_string(b) + "] = " + std::to_string(n_out[b]);
    if (len > max) return std::string(name) + " = " + std::to_string(len) + " is above 2^30 = " + std::to_string(max);
    return std::string();
}

// Every launch's own tile numbering: over tiles = segment_launches(S) zeros, called for s = 0 .. S - 1 in order with the n tiles of
// segment s, it returns the segment's first tile in its launch, and tiles[l] ends as the workgroups of launch l.
inline int32_t segment_take_tiles(std::vector<int64_t>& tiles, int s, int64_t n) {
    int64_t& t = tiles[(size_t)(s / SEGMENTS_PER_LAUNCH)];
    t += n;
    return (int32_t)(t - n);
}

// Cuts the entries of a call into launches: launch(c, n, l) gets launch l's chunk -- its n entries, and `pad` behind them -- and
// returns 0 to go on; the first other value ends the walk and is returned.
template <class Entry, class Launch>
inline int for_each_segment_launch(const std::vector<Entry>& entries, const Entry& pad, Launch launch) {
    const int S = (int)entries.size();
    for (int s0 = 0, l = 0; s0 < S; s0 += SEGMENTS_PER_LAUNCH, ++l) {
        const int n = S - s0 < SEGMENTS_PER_LAUNCH ? S - s0 : SEGMENTS_PER_LAUNCH;
        SegmentChunk<Entry> c;
        for (int q = 0; q < SEGMENTS_PER_LAUNCH; ++q) c.e[q] = q < n ? entries[(size_t)s0 + q] : pad;
        const int rc = launch(c, n, l);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace tts
