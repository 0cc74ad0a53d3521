// Formant-preserving pitch, host side: the checks of a shift's segment list, how the list is cut into launches and tiles, the
// cosine table and the lifter, and the kernel's LDS layout (host, kernel and tests/shift_oracle.py share this one definition).
// Plain C++ (no HIP, no handle): shift.hip includes it, and tests/shift_check.cpp compiles it alone.
//
// The cut: every frame of out[B][F][T] is OWNED by exactly one segment.  Segment s of a row owns [lead, end): the uncovered frames
// between its predecessor's end (or frame 0) and its own first frame, then its own frames [first, end); a row's last segment
// owns the row's rest [end, T) as well.  What a segment owns falls into three runs of tiles, numbered in this order:
//   lead   [lead, first)   copies, SHIFT_COPY_TILE frames per workgroup
//   body   [first, end)    SHIFT_TILE frames per workgroup where the segment is computed; a segment whose two steps are both
//                          65536 is a copy and takes SHIFT_COPY_TILE frames per workgroup
//   rest   [end, own_end)  copies below n_frames[row], +0.0 from there on, SHIFT_COPY_TILE frames per workgroup
// segments.h has the list's order, the launches and the numbering of their tiles.  The launches of a call write disjoint ranges
// that cover out: every element once.
#pragma once
#include "segments.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sstts_hip.h"

namespace tts {

constexpr int SHIFT_SEGMENTS = SEGMENTS_PER_LAUNCH, SHIFT_MAX_SEGMENTS = MAX_SEGMENTS;
constexpr int SHIFT_THREADS = 512;
constexpr int SHIFT_TILE = 8;                // frames of a computed segment one workgroup takes
constexpr int SHIFT_COPY_TILE = 64;          // frames of a copied run one workgroup takes: a wave along the frames
constexpr int SHIFT_MAX_ORDER = 256;
constexpr int SHIFT_N_MIN = 128, SHIFT_N_MAX = 2048;
constexpr uint32_t SHIFT_UNITY = 65536, SHIFT_STEP_MIN = 32768, SHIFT_STEP_MAX = 131072;   // one octave either way
constexpr int SHIFT_PARTS = 8;               // the lanes that share one cepstral sum: lane p takes the bins k = 8 j + p
constexpr int SHIFT_LDS_FLOATS_PER_PASS = 8 * 1032;   // the frames of a pass times their padded row: 8 at N <= 1024, 4 at N = 2048

constexpr int shift_launches(int S) { return segment_launches(S); }
constexpr int64_t shift_tiles(int64_t frames, int tile) { return (frames + tile - 1) / tile; }

// ---- the LDS image of a compute workgroup.  A frame's row is N + 8 elements: 8 (mod 32) doubles, so that the 8 frames x 4 bins (or
// x 8 parts) of a half-wave's 8-byte reads lie on 32 distinct bank pairs.  The cosine table is padded by one double per 32, so that
// a stride of 16 or 32 entries (q = 16, 32, ...) does not land every lane on one bank: entry j sits at j + (j >> 5).
constexpr int shift_row(int N) { return N + 8; }
constexpr int shift_pass_frames(int N) { return SHIFT_LDS_FLOATS_PER_PASS / shift_row(N) < SHIFT_TILE ? SHIFT_LDS_FLOATS_PER_PASS / shift_row(N) : SHIFT_TILE; }
constexpr int shift_ct_slot(int j) { return j + (j >> 5); }
constexpr int shift_ct_doubles(int N) { return 2 * N + (2 * N >> 5); }
// ct [shift_ct_doubles], LE [pass][row] double, hc [Q][pass] double, xs [pass][row] float, bad [SHIFT_TILE] int
constexpr size_t shift_lds_bytes(int N, int Q) {
    return sizeof(double) * ((size_t)shift_ct_doubles(N) + (size_t)shift_pass_frames(N) * shift_row(N) + (size_t)Q * shift_pass_frames(N)) +
           sizeof(float) * (size_t)shift_pass_frames(N) * shift_row(N) + sizeof(int) * SHIFT_TILE;
}
constexpr size_t SHIFT_LDS_LIMIT = 160 * 1024;
static_assert(shift_pass_frames(1024) == 8 && shift_pass_frames(2048) == 4 && shift_pass_frames(128) == 8, "frames of a pass");
static_assert(shift_lds_bytes(2048, SHIFT_MAX_ORDER) <= SHIFT_LDS_LIMIT && shift_lds_bytes(1024, SHIFT_MAX_ORDER) <= SHIFT_LDS_LIMIT, "LDS of a workgroup");

// F = N + 1 with N a power of two in SHIFT_N_MIN .. SHIFT_N_MAX: N, else 0
constexpr int shift_bins_n(int F) {
    return (F - 1 >= SHIFT_N_MIN && F - 1 <= SHIFT_N_MAX && ((F - 1) & (F - 2)) == 0) ? F - 1 : 0;
}

// ct[j] = cos(pi j / N), j < 2N, in double (unpadded: the kernel's copy is laid out by shift_ct_slot)
inline std::vector<double> shift_cos_table(int N) {
    std::vector<double> ct((size_t)2 * N);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < 2 * N; ++j) ct[(size_t)j] = std::cos(pi * (double)j / (double)N);
    return ct;
}
inline std::vector<double> shift_cos_table_padded(int N) {
    const std::vector<double> ct = shift_cos_table(N);
    std::vector<double> p((size_t)shift_ct_doubles(N), 0.0);
    for (int j = 0; j < 2 * N; ++j) p[(size_t)shift_ct_slot(j)] = ct[(size_t)j];
    return p;
}
// the raised-cosine lifter: h[0] = 1, h[q] = 1 + cos(pi q / Q)
inline std::vector<double> shift_lifter(int Q) {
    std::vector<double> h((size_t)Q);
    const double pi = 3.14159265358979323846;
    for (int q = 0; q < Q; ++q) h[(size_t)q] = q == 0 ? 1.0 : 1.0 + std::cos(pi * (double)q / (double)Q);
    return h;
}

// What the kernel knows of a segment: its row, the frames it owns ([lead, own_end), of which [first, end) are its own), the frames
// of its row that hold data, its two steps and its first tile in the launch.
struct ShiftEntry {
    int32_t row, lead, first, end, own_end, n, tile0;
    uint32_t pitch_step, formant_step;
};
using ShiftChunk = SegmentChunk<ShiftEntry>;
constexpr ShiftEntry SHIFT_NO_ENTRY{0, 0, 0, 0, 0, 0, 0, SHIFT_UNITY, SHIFT_UNITY};   // a copy of nothing: what pads a launch's chunk
constexpr bool shift_is_copy(uint32_t pitch_step, uint32_t formant_step) { return pitch_step == SHIFT_UNITY && formant_step == SHIFT_UNITY; }
inline int64_t shift_lead_tiles(const ShiftEntry& w) { return shift_tiles((int64_t)w.first - w.lead, SHIFT_COPY_TILE); }
inline int64_t shift_body_tiles(const ShiftEntry& w) {
    return shift_tiles((int64_t)w.end - w.first, shift_is_copy(w.pitch_step, w.formant_step) ? SHIFT_COPY_TILE : SHIFT_TILE);
}
inline int64_t shift_rest_tiles(const ShiftEntry& w) { return shift_tiles((int64_t)w.own_end - w.end, SHIFT_COPY_TILE); }

// The checks of tts_shift_plan and tts_shift_magnitudes on the shape and the list, in the order the header lists them.  An empty
// string: legal (TTS_ERR_INVALID otherwise).
inline std::string shift_plan(const tts_shift_segment_t* seg, int S, int B, int F, int T, const int32_t* n_frames, int order) {
    if (!seg) return "a NULL pointer (segments are required)";
    if (B < 1 || T < 1 || S < 1) return "need B, T, S >= 1";
    const int N = shift_bins_n(F);
    if (!N) return "F = " + std::to_string(F) + " is not 2^m + 1 with 2^m in " + std::to_string(SHIFT_N_MIN) + " .. " + std::to_string(SHIFT_N_MAX);
    const int order_max = SHIFT_MAX_ORDER < N / 2 ? SHIFT_MAX_ORDER : N / 2;
    if (order < 2 || order > order_max) return "order = " + std::to_string(order) + " is not in 2 .. " + std::to_string(order_max);
    const std::string bad = segment_rows_refusal(seg, S, B, "tts_shift_max_segments()", "n_frames", n_frames, "T", T);
    if (!bad.empty()) return bad;
    int64_t prev_end = 0;
    for (int s = 0; s < S; ++s) {
        const tts_shift_segment_t& q = seg[s];
        const std::string name = "segment " + std::to_string(s);
        if (s > 0 && seg[s - 1].row != q.row) prev_end = 0;
        if (q.frames < 1) return name + " has " + std::to_string(q.frames) + " frames: at least 1 is needed";
        const int n = n_frames ? n_frames[q.row] : T;
        if (q.first < 0 || (int64_t)q.first + q.frames > (int64_t)n)
            return name + " covers frames " + std::to_string(q.first) + " .. " + std::to_string((int64_t)q.first + q.frames - 1) + " of row " +
                   std::to_string(q.row) + ", which has 0 .. " + std::to_string(n - 1);
        if ((int64_t)q.first < prev_end)
            return name + " starts at frame " + std::to_string(q.first) + " of row " + std::to_string(q.row) + ", in front of its predecessor's end " +
                   std::to_string(prev_end) + ": the ranges of a row ascend and do not overlap";
        if (q.reserved != 0) return name + " has reserved = " + std::to_string(q.reserved) + ", which must be 0";
        if (q.pitch_step < SHIFT_STEP_MIN || q.pitch_step > SHIFT_STEP_MAX)
            return name + " has pitch_step " + std::to_string(q.pitch_step) + ", which is not in " + std::to_string(SHIFT_STEP_MIN) + " .. " +
                   std::to_string(SHIFT_STEP_MAX);
        if (q.formant_step < SHIFT_STEP_MIN || q.formant_step > SHIFT_STEP_MAX)
            return name + " has formant_step " + std::to_string(q.formant_step) + ", which is not in " + std::to_string(SHIFT_STEP_MIN) + " .. " +
                   std::to_string(SHIFT_STEP_MAX);
        prev_end = (int64_t)q.first + q.frames;
    }
    return std::string();
}

// The entries of a legal list with every launch's own tile numbering: entry s is segment s, and tiles[l] the workgroups of launch l.
inline void shift_entries(const tts_shift_segment_t* seg, int S, int T, const int32_t* n_frames, std::vector<ShiftEntry>& e, std::vector<int64_t>& tiles) {
    e.assign((size_t)S, SHIFT_NO_ENTRY);
    tiles.assign((size_t)segment_launches(S), 0);
    int32_t prev_end = 0;
    for (int s = 0; s < S; ++s) {
        const tts_shift_segment_t& q = seg[s];
        if (s > 0 && seg[s - 1].row != q.row) prev_end = 0;
        const bool last = s + 1 == S || seg[s + 1].row != q.row;
        ShiftEntry& w = e[(size_t)s];
        w.row = q.row;
        w.lead = prev_end;
        w.first = q.first;
        w.end = q.first + q.frames;
        w.own_end = last ? T : w.end;
        w.n = n_frames ? n_frames[q.row] : T;
        w.pitch_step = q.pitch_step;
        w.formant_step = q.formant_step;
        w.tile0 = segment_take_tiles(tiles, s, shift_lead_tiles(w) + shift_body_tiles(w) + shift_rest_tiles(w));
        prev_end = w.end;
    }
}

// What tile `tile` of entry w (numbered from the entry's first) is: the frames [t0, t1) and whether they are computed.
struct ShiftTile {
    int32_t t0, t1;
    bool compute;
};
inline
#ifdef __HIPCC__
    __host__ __device__
#endif
    ShiftTile
    shift_tile_of(const ShiftEntry& w, int tile) {
    const int lead = (w.first - w.lead + SHIFT_COPY_TILE - 1) / SHIFT_COPY_TILE;
    const bool copy = w.pitch_step == SHIFT_UNITY && w.formant_step == SHIFT_UNITY;
    const int bt = copy ? SHIFT_COPY_TILE : SHIFT_TILE;
    const int body = (w.end - w.first + bt - 1) / bt;
    ShiftTile r;
    if (tile < lead) {
        r.t0 = w.lead + tile * SHIFT_COPY_TILE;
        r.t1 = r.t0 + SHIFT_COPY_TILE < w.first ? r.t0 + SHIFT_COPY_TILE : w.first;
        r.compute = false;
    } else if (tile < lead + body) {
        r.t0 = w.first + (tile - lead) * bt;
        r.t1 = r.t0 + bt < w.end ? r.t0 + bt : w.end;
        r.compute = !copy;
    } else {
        r.t0 = w.end + (tile - lead - body) * SHIFT_COPY_TILE;
        r.t1 = r.t0 + SHIFT_COPY_TILE < w.own_end ? r.t0 + SHIFT_COPY_TILE : w.own_end;
        r.compute = false;
    }
    return r;
}

}  // namespace tts
