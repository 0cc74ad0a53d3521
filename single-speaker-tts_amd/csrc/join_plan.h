// The join of waveform pieces, host side: the checks of an edit list, where every piece lands in its group's row, the fade of a
// piece's edges (host, kernel and tests/join_oracle.py share this one definition) and how the list is cut into launches.  Plain
// C++ (no HIP, no handle): join.hip includes it, and tests/join_check.cpp compiles it alone.
//
// The layout of a group: piece p starts at o[p]; o of a group's first piece is 0, o[p+1] = o[p] + count[p] + gap[p], and the group is
// n_out = o[last] + count[last] samples long.  A negative gap lays the head of piece p+1 over the tail of piece p.
//
// The cut: every output sample is OWNED by exactly one piece -- piece p owns [o[p], o[p+1]) of its group's row, a group's last piece
// [o[p], N_out).  -gap[p] <= min(f_p, f_p+1) <= count / 2 makes these ranges non-empty and ascending.  What a piece owns holds its own
// samples from its start on (without the tail the next piece lies over), in front the tail of its predecessor where that one lies over
// its head, and behind its end the zeros of its gap (or of the row's rest).  In the flat array out[G * N_out] the owned ranges are one
// ascending partition, so a launch that takes JOIN_PIECES consecutive pieces writes one contiguous range, and the launches of a call
// write disjoint ranges that cover the array: every element once.
#pragma once
#include "lengths.h"
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sstts_hip.h"

namespace tts {

constexpr int JOIN_PIECES = 128;            // pieces per launch: their entries travel by value
constexpr int JOIN_MAX_PIECES = 4096;       // pieces per call (32 launches)
constexpr int JOIN_MAX_FADE = 1 << 20;      // samples: 2 i + 1 and 2 f stay far inside int32
constexpr int JOIN_THREADS = 128;
constexpr int JOIN_TILE = 4 * JOIN_THREADS; // output samples of a workgroup: one aligned 16-byte store per thread

constexpr int join_launches(int P) { return (P + JOIN_PIECES - 1) / JOIN_PIECES; }

// (constexpr: the kernel calls these too)
constexpr int join_fade(int fade, int count) { return fade < count / 2 ? fade : count / 2; }
constexpr double join_s(double t) { return (t * t) * (3.0 - 2.0 * t); }
// the gain of sample i of a piece of `count` samples that fades over f = join_fade(fade, count)
constexpr double join_gain(int i, int count, int f) {
    if (i < f) return join_s((double)(2 * i + 1) / (double)(2 * f));
    if (i >= count - f) return join_s((double)(2 * (count - 1 - i) + 1) / (double)(2 * f));
    return 1.0;
}

// What the kernel knows of a piece: where its owned range starts in the flat output, its samples, and how many samples of its
// predecessor's tail lie over its head (0: none, or the first piece of a group).
struct JoinEntry {
    int64_t start;
    int32_t row, first, count, over;
};
// A launch: e[0] is the predecessor of the launch's first piece (read only where e[1].over > 0), e[1 .. n] its pieces.
struct JoinChunk {
    JoinEntry e[JOIN_PIECES + 1];
};

// The checks of tts_join_plan and tts_join on the list, in the order the header lists them, and the layout.  An empty string: the
// list is legal (TTS_ERR_INVALID otherwise).  n_out [G], offset [P] and f [P] are filled where they are given.
inline std::string join_plan(const tts_join_piece_t* pieces, int P, const int32_t* group, int G, int B, int N, int fade, int64_t* n_out,
                             int64_t* offset = nullptr, int32_t* f = nullptr) {
    if (!pieces || !group || !n_out) return "a NULL pointer (pieces, group and n_out are required)";
    if (B < 1 || N < 1 || P < 1 || G < 1) return "need B, N, P, G >= 1";
    if (G > P) return std::to_string(G) + " groups of " + std::to_string(P) + " pieces: no group is empty";
    if (fade < 0) return "fade < 0";
    if (fade > JOIN_MAX_FADE) return "fade = " + std::to_string(fade) + " is larger than tts_join_max_fade() = " + std::to_string(JOIN_MAX_FADE);
    if (P > JOIN_MAX_PIECES)
        return std::to_string(P) + " pieces are more than tts_join_max_pieces() = " + std::to_string(JOIN_MAX_PIECES);
    for (int p = 0; p < P; ++p) {
        const tts_join_piece_t& q = pieces[p];
        if (q.row < 0 || q.row >= B) return "row[" + std::to_string(p) + "] = " + std::to_string(q.row) + " is not in 0 .. B - 1 = " + std::to_string(B - 1);
        if (q.first < 0 || q.first >= N)
            return "first[" + std::to_string(p) + "] = " + std::to_string(q.first) + " is not in 0 .. N - 1 = " + std::to_string(N - 1);
        const std::string bad = length_refusal("count", p, q.count, "N - first", N - q.first);
        if (!bad.empty()) return bad;
    }
    if (group[0] != 0) return "group[0] = " + std::to_string(group[0]) + ": the groups start at 0";
    for (int p = 1; p < P; ++p)
        if (group[p] != group[p - 1] && group[p] != group[p - 1] + 1)
            return "group[" + std::to_string(p) + "] = " + std::to_string(group[p]) + " follows " + std::to_string(group[p - 1]) +
                   ": the groups are non-decreasing and none is empty";
    if (group[P - 1] != G - 1) return "group[" + std::to_string(P - 1) + "] = " + std::to_string(group[P - 1]) + ": the last group is G - 1 = " + std::to_string(G - 1);
    int64_t o = 0;
    for (int p = 0; p < P; ++p) {
        const int fp = join_fade(fade, pieces[p].count);
        if (offset) offset[p] = o;
        if (f) f[p] = fp;
        if (p + 1 == P || group[p + 1] != group[p]) {   // (the gap of a group's last piece is ignored)
            n_out[group[p]] = o + pieces[p].count;
            o = 0;
            continue;
        }
        const int fn = join_fade(fade, pieces[p + 1].count);
        const int room = fp < fn ? fp : fn;
        if ((int64_t)pieces[p].gap < -(int64_t)room)
            return "gap[" + std::to_string(p) + "] = " + std::to_string(pieces[p].gap) + " overlaps more than min(f[" + std::to_string(p) + "], f[" +
                   std::to_string(p + 1) + "]) = " + std::to_string(room) + " samples";
        o += (int64_t)pieces[p].count + pieces[p].gap;
    }
    return std::string();
}

// the most output samples G * N_out of a call: a launch covers at most that many, and its grid of workgroups times JOIN_THREADS stays
// below 2^32, which is what a launch takes
constexpr int64_t JOIN_MAX_SAMPLES = (int64_t)1 << 33;

// ... and of tts_join's own arguments behind a legal list
inline std::string join_room(const int64_t* n_out, int G, int N_out) {
    for (int g = 0; g < G; ++g)
        if (n_out[g] > (int64_t)N_out)
            return "N_out = " + std::to_string(N_out) + " is below n_out[" + std::to_string(g) + "] = " + std::to_string(n_out[g]);
    if ((int64_t)G * N_out > JOIN_MAX_SAMPLES)
        return "G * N_out = " + std::to_string((int64_t)G * N_out) + " output samples are more than 2^33 = " + std::to_string(JOIN_MAX_SAMPLES);
    return std::string();
}

// The entries of a legal list (offset from join_plan): entry p + 1 is piece p, entry 0 is unused.
inline void join_entries(const tts_join_piece_t* pieces, int P, const int32_t* group, int N_out, const int64_t* offset, std::vector<JoinEntry>& e) {
    e.assign((size_t)P + 1, JoinEntry{0, 0, 0, 0, 0});
    for (int p = 0; p < P; ++p) {
        JoinEntry& q = e[(size_t)p + 1];
        q.start = (int64_t)group[p] * N_out + offset[p];
        q.row = pieces[p].row;
        q.first = pieces[p].first;
        q.count = pieces[p].count;
        q.over = (p > 0 && group[p - 1] == group[p] && pieces[p - 1].gap < 0) ? -pieces[p - 1].gap : 0;
    }
}

}  // namespace tts
