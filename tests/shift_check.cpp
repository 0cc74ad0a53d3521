// Stand-alone check of the host side of the formant-preserving pitch stage (csrc/shift_plan.h compiled as plain C++, no GPU, no
// library): prints the constants, the LDS of a workgroup, the cut of a table of segment lists into launches and tiles, samples of
// the cosine table and the lifter, and what the plan answers to a list of bad argument sets, for tests/test_shift_program.py to
// hold against tests/shift_oracle.py.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "shift_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

struct List {
    const char* name;
    int B, F, T, order;
    std::vector<int32_t> n_frames;   // empty: all T
    std::vector<tts_shift_segment_t> seg;
};

static std::string g_why;

// 0: legal, 1: TTS_ERR_INVALID
static int answer(const List& l, bool ptrs = true) {
    g_why = shift_plan(ptrs ? l.seg.data() : nullptr, (int)l.seg.size(), l.B, l.F, l.T, l.n_frames.empty() ? nullptr : l.n_frames.data(), l.order);
    return g_why.empty() ? 0 : 1;
}

static void bad(const char* name, const List& l, bool ptrs = true) {
    std::printf("check %s %d\n", name, answer(l, ptrs));
    std::printf("msg %s %s\n", name, g_why.c_str());
}

// the list and its cut: every frame of every row has exactly one owner, and a computed tile lies inside its segment
static void show(const List& l) {
    const int S = (int)l.seg.size();
    const int32_t* nf = l.n_frames.empty() ? nullptr : l.n_frames.data();
    expect(answer(l) == 0, l.name);
    if (!g_why.empty()) return;
    std::printf("list %s %d %d %d %d\n", l.name, l.B, l.F, l.T, S);
    for (int b = 0; b < l.B; ++b) std::printf("frames %s %d %d\n", l.name, b, nf ? nf[b] : l.T);
    for (int s = 0; s < S; ++s)
        std::printf("seg %s %d %d %d %d %u %u\n", l.name, s, l.seg[s].row, l.seg[s].first, l.seg[s].frames, l.seg[s].pitch_step, l.seg[s].formant_step);
    std::vector<ShiftEntry> e;
    std::vector<int64_t> tiles;
    shift_entries(l.seg.data(), S, l.T, nf, e, tiles);
    expect((int)e.size() == S && (int)tiles.size() == shift_launches(S), "an entry per segment, a tile count per launch");
    std::vector<std::vector<int>> owners((size_t)l.B, std::vector<int>((size_t)l.T, 0));
    for (int s = 0; s < S; ++s) {
        const ShiftEntry& w = e[(size_t)s];
        const int lead = (int)shift_lead_tiles(w), body = (int)shift_body_tiles(w), rest = (int)shift_rest_tiles(w);
        std::printf("entry %s %d %d %d %d %d %d\n", l.name, s, s / SHIFT_SEGMENTS, w.tile0, lead, body, rest);
        expect(0 <= w.lead && w.lead <= w.first && w.first < w.end && w.end <= w.n && w.n <= l.T && w.end <= w.own_end && w.own_end <= l.T,
               "what a segment owns lies inside its row");
        const bool copy = shift_is_copy(w.pitch_step, w.formant_step);
        for (int t = 0; t < lead + body + rest; ++t) {
            const ShiftTile k = shift_tile_of(w, t);
            expect(k.t0 < k.t1 && k.t0 >= w.lead && k.t1 <= w.own_end, "a tile lies inside what its segment owns");
            expect(k.compute == (!copy && t >= lead && t < lead + body), "the body of a segment that is no copy is computed, nothing else");
            if (k.compute) expect(k.t0 >= w.first && k.t1 <= w.end && k.t1 - k.t0 <= SHIFT_TILE, "a computed tile lies inside its segment");
            else expect(k.t1 - k.t0 <= SHIFT_COPY_TILE, "a copy tile is one wave of frames");
            for (int f = k.t0; f < k.t1; ++f) ++owners[(size_t)w.row][(size_t)f];
        }
    }
    bool once = true;
    for (const auto& row : owners)
        for (int c : row) once = once && c == 1;
    expect(once, "every frame of out has exactly one owner");
    for (size_t k = 0; k < tiles.size(); ++k) std::printf("tiles %s %d %lld\n", l.name, (int)k, (long long)tiles[k]);
}

int main() {
    std::printf("consts %d %d %d %d %d %d %u %u %d %d\n", SHIFT_SEGMENTS, SHIFT_MAX_SEGMENTS, SHIFT_THREADS, SHIFT_TILE, SHIFT_COPY_TILE, SHIFT_MAX_ORDER,
                SHIFT_STEP_MIN, SHIFT_STEP_MAX, SHIFT_N_MIN, SHIFT_N_MAX);
    expect(sizeof(tts_shift_segment_t) == 24, "a segment is four int32 and two uint32");
    expect(sizeof(ShiftEntry) == 36 && sizeof(ShiftChunk) + 64 <= 3800, "a launch's entries fit the kernel's argument space");
    expect(SHIFT_THREADS % (SHIFT_PARTS * SHIFT_TILE) == 0 && SHIFT_THREADS % 64 == 0, "whole groups of lanes per sum, whole waves per bin");
    for (int S : {1, 63, 64, 65, 4096}) std::printf("launches %d %d\n", S, shift_launches(S));
    for (int N = SHIFT_N_MIN; N <= SHIFT_N_MAX; N *= 2) {
        expect(shift_bins_n(N + 1) == N && shift_bins_n(N) == 0 && shift_bins_n(N + 2) == 0, "F = 2^m + 1");
        expect(shift_row(N) % 32 == 8, "a frame's row is 8 (mod 32) elements: conflict-free 8-byte reads across the frames of a pass");
        for (int Q : {2, 33, N / 2 < SHIFT_MAX_ORDER ? N / 2 : SHIFT_MAX_ORDER}) {
            std::printf("lds %d %d %d %zu\n", N, Q, shift_pass_frames(N), shift_lds_bytes(N, Q));
            expect(shift_lds_bytes(N, Q) <= SHIFT_LDS_LIMIT, "a workgroup's LDS fits a compute unit's 160 KB");
        }
        expect(SHIFT_TILE % shift_pass_frames(N) == 0 && (shift_pass_frames(N) & (shift_pass_frames(N) - 1)) == 0, "whole passes per tile, a power of two");
    }
    expect(shift_bins_n(65) == 0 && shift_bins_n(4097) == 0 && shift_bins_n(1) == 0 && shift_bins_n(0) == 0 && shift_bins_n(-5) == 0, "N in 128 .. 2048");
    {   // the tables: samples in hex floats, and the padded image
        const std::vector<double> ct = shift_cos_table(128), pad = shift_cos_table_padded(128), h = shift_lifter(33);
        for (int j : {0, 1, 64, 127, 128, 255}) std::printf("ct 128 %d %a\n", j, ct[(size_t)j]);
        for (int q : {0, 1, 16, 32}) std::printf("lifter 33 %d %a\n", q, h[(size_t)q]);
        bool same = (int)pad.size() == shift_ct_doubles(128) && shift_ct_slot(255) < shift_ct_doubles(128);
        for (int j = 0; j < 256; ++j) same = same && pad[(size_t)shift_ct_slot(j)] == ct[(size_t)j];
        expect(same, "the padded table holds every entry at its slot");
    }

    const uint32_t U = SHIFT_UNITY;
    const std::vector<List> lists = {
        {"one", 1, 129, 10, 2, {}, {{0, 0, 10, 0, 49152, U}}},
        {"seam", 1, 1025, 70, 33, {}, {{0, 2, SHIFT_TILE - 1, 0, 52016, U}, {0, 9, SHIFT_TILE, 0, U, 77936}, {0, 20, SHIFT_TILE + 1, 0, 82570, 58386},
                                      {0, 29, 5, 0, U, U}, {0, 34, 17, 0, SHIFT_STEP_MIN, SHIFT_STEP_MAX}}},
        {"ragged", 3, 2049, 200, 64, {200, 41, 9}, {{0, 70, 3, 0, 52016, U}, {0, 140, 60, 0, U, U}, {1, 0, 41, 0, 52016, U}, {2, 3, 1, 0, 73562, 73562}}},
    };
    for (const List& l : lists) show(l);
    {   // a list one longer than a launch carries, with a row whose segments straddle two launches
        List l{"straddle", 2, 1025, 70, 33, {70, 66}, {}};
        for (int s = 0; s < SHIFT_SEGMENTS - 4; ++s) l.seg.push_back({0, s, 1, 0, s % 3 ? 52016u : U, s % 5 ? U : 77936u});
        for (int j = 0; j < 5; ++j) l.seg.push_back({1, 2 + 12 * j, 1 + 2 * j, 0, 82570, U});
        show(l);
    }

    const List ok = lists[2];
    std::printf("check legal %d\n", answer(ok));
    bad("null", ok, false);
    { List l = ok; l.B = 0; bad("B0", l); }
    { List l = ok; l.T = 0; bad("T0", l); }
    { List l = ok; l.seg.clear(); bad("S0", l); }
    { List l = ok; l.F = 2048; bad("F_even", l); }
    { List l = ok; l.F = 65; bad("F_small", l); }
    { List l = ok; l.F = 4097; bad("F_large", l); }
    { List l = ok; l.order = 1; bad("order_low", l); }
    { List l = ok; l.order = 257; bad("order_high", l); }
    { List l = ok; l.F = 129; l.order = 65; bad("order_half_n", l); }
    { List l = ok; l.F = 129; l.order = 64; std::printf("check legal_order %d\n", answer(l)); }
    { List l = ok; l.F = 4097; l.B = 0; bad("B_before_F", l); }
    { List l = ok; l.F = 65; l.order = 0; bad("F_before_order", l); }
    {
        List l{"many", 1, 129, 4100, 2, {}, {}};
        for (int s = 0; s < SHIFT_MAX_SEGMENTS; ++s) l.seg.push_back({0, s, 1, 0, U, U});
        std::printf("check legal_max_segments %d\n", answer(l));
        l.seg.push_back({0, 4096, 1, 0, U, U});
        bad("segments_max", l);
        l.order = 1;
        bad("order_before_segments_max", l);
    }
    { List l = ok; l.B = 10; l.n_frames.assign(10, 7); bad("rows_over_segments", l); }
    { List l = ok; l.B = 2147483647; bad("Bmax", l); }
    for (int v : {0, -1, 201}) {
        List l = ok;
        l.n_frames[1] = v;
        std::printf("check n_frames=%d %d\n", v, answer(l));
        std::printf("msg n_frames=%d %s\n", v, g_why.c_str());
    }
    { List l = ok; l.seg[0].row = 1; bad("row_start", l); }
    { List l = ok; l.seg[3].row = 0; bad("row_back", l); }
    { List l = ok; l.seg[2].row = 0; bad("row_skip", l); }
    { List l = ok; l.B = 4; l.n_frames.push_back(5); bad("row_end", l); }
    { List l = ok; l.seg[1].row = -1; bad("row_negative", l); }
    { List l = ok; l.seg[1].frames = 0; bad("frames0", l); }
    { List l = ok; l.seg[1].frames = -3; bad("frames-3", l); }
    { List l = ok; l.seg[1].frames = 61; bad("past_the_row", l); }
    { List l = ok; l.seg[2].frames = 42; bad("past_n_frames", l); }
    { List l = ok; l.seg[0].first = -1; bad("first-1", l); }
    { List l = ok; l.seg[1].first = 2147483647; bad("first_max", l); }   // (first + frames in 64 bits)
    { List l = ok; l.seg[1].first = 72; bad("overlap", l); }
    { List l = ok; l.seg[1].first = 10; bad("precedes", l); }
    { List l = ok; l.seg[1].first = 73; std::printf("check legal_adjacent %d\n", answer(l)); }
    { List l = ok; l.seg[3].reserved = 1; bad("reserved", l); }
    { List l = ok; l.seg[3].reserved = 1; l.seg[3].first = 9; bad("range_before_reserved", l); }
    { List l = ok; l.seg[0].pitch_step = SHIFT_STEP_MIN - 1; bad("pitch_low", l); }
    { List l = ok; l.seg[0].pitch_step = SHIFT_STEP_MAX + 1; bad("pitch_high", l); }
    { List l = ok; l.seg[0].formant_step = SHIFT_STEP_MIN - 1; bad("formant_low", l); }
    { List l = ok; l.seg[0].formant_step = SHIFT_STEP_MAX + 1; bad("formant_high", l); }
    { List l = ok; l.seg[0].formant_step = 0; l.seg[0].reserved = 7; bad("reserved_before_steps", l); }
    { List l = ok; l.seg[0].pitch_step = SHIFT_STEP_MIN; l.seg[0].formant_step = SHIFT_STEP_MAX; std::printf("check legal_steps %d\n", answer(l)); }
    // the largest grid is a legal launch: 64 segments of a row of 2^27 frames are fewer than 2^31 tiles
    expect((int64_t)SHIFT_SEGMENTS * (shift_tiles((int64_t)1 << 27, SHIFT_TILE) + 2) < ((int64_t)1 << 31), "the largest grid is a legal launch");
    return exit_status();
}
