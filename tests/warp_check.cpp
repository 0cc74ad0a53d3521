// Stand-alone check of the host side of the prosody warp (csrc/warp_plan.h compiled as plain C++, no GPU, no library): prints the
// constants, the output frames of every segment and row of a table of segment lists, the cut of each into launches and tiles, and
// what the plan answers to a list of bad argument sets, for tests/test_warp_program.py to hold against tests/warp_oracle.py.
// Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "warp_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

struct List {
    const char* name;
    int B, T;
    std::vector<int32_t> n_frames;   // empty: all T
    std::vector<tts_warp_segment_t> seg;
};

static std::string g_why;

// 0: legal, 1: TTS_ERR_INVALID
static int answer(const List& l, bool ptrs = true) {
    std::vector<int64_t> n_out((size_t)(l.B > 0 && l.B <= WARP_MAX_SEGMENTS ? l.B : 1));   // (more rows than segments: refused before a length is written)
    g_why = warp_plan(ptrs ? l.seg.data() : nullptr, (int)l.seg.size(), l.B, l.T, l.n_frames.empty() ? nullptr : l.n_frames.data(), n_out.data());
    return g_why.empty() ? 0 : 1;
}

static void bad(const char* name, const List& l, bool ptrs = true) {
    std::printf("check %s %d\n", name, answer(l, ptrs));
    std::printf("msg %s %s\n", name, g_why.c_str());
}

// the list, its lengths and its cut at T_out = the longest row + extra
static void show(const List& l, int extra) {
    const int S = (int)l.seg.size();
    std::vector<int64_t> n_out((size_t)l.B), count((size_t)S);
    const int32_t* nf = l.n_frames.empty() ? nullptr : l.n_frames.data();
    const std::string why = warp_plan(l.seg.data(), S, l.B, l.T, nf, n_out.data(), count.data());
    expect(why.empty(), l.name);
    if (!why.empty()) return;
    int64_t longest = 0;
    for (int64_t n : n_out) longest = n > longest ? n : longest;
    const int T_out = (int)longest + extra;
    std::printf("list %s %d %d %d %d\n", l.name, l.B, l.T, S, T_out);
    for (int b = 0; b < l.B; ++b) std::printf("frames %s %d %d\n", l.name, b, nf ? nf[b] : l.T);
    for (int s = 0; s < S; ++s)
        std::printf("seg %s %d %d %d %d %d %u %.9g %lld\n", l.name, s, l.seg[s].row, l.seg[s].first, l.seg[s].frames, l.seg[s].pause, l.seg[s].step,
                    (double)l.seg[s].gain, (long long)count[s]);
    for (int b = 0; b < l.B; ++b) std::printf("n_out %s %d %lld\n", l.name, b, (long long)n_out[b]);
    expect(warp_room(n_out.data(), l.B, T_out).empty() && !warp_room(n_out.data(), l.B, (int)longest - 1).empty(), "the room is the longest row");
    std::vector<WarpEntry> e;
    std::vector<int64_t> tiles;
    warp_entries(l.seg.data(), S, l.T, nf, T_out, count.data(), e, tiles);
    expect((int)e.size() == S && (int)tiles.size() == warp_launches(S), "an entry per segment, a tile count per launch");
    for (int s = 0; s < S; ++s) {
        const WarpEntry& w = e[(size_t)s];
        std::printf("entry %s %d %d %d %d %d %d %d\n", l.name, s, s / WARP_SEGMENTS, w.tile0, (int)warp_tiles(w.span), w.o, w.count, w.span);
        expect(w.span >= 1 && w.count <= w.span && (int64_t)w.o + w.span <= T_out, "what a segment owns lies inside its row");
        expect(w.count == 0 || (w.first >= 0 && (int64_t)w.first + ((((int64_t)w.count - 1) * w.step) >> 16) < w.n), "the last blended frame reads inside the row");
    }
    for (size_t k = 0; k < tiles.size(); ++k) std::printf("tiles %s %d %lld\n", l.name, (int)k, (long long)tiles[k]);
}

int main() {
    std::printf("consts %d %d %d %d %d %u %u\n", WARP_SEGMENTS, WARP_MAX_SEGMENTS, WARP_THREADS, WARP_TILE, WARP_BINS, WARP_STEP_MIN, WARP_STEP_MAX);
    expect(sizeof(tts_warp_segment_t) == 24, "a segment is four int32, a uint32 and a float");
    expect(sizeof(WarpEntry) == 36 && sizeof(WarpChunk) + 64 <= 3800, "a launch's entries fit the kernel's argument space");
    expect(WARP_THREADS % WARP_TILE == 0 && WARP_TILE == 64 && WARP_BINS % (WARP_THREADS / WARP_TILE) == 0, "a wave along the frames, whole rounds of bins");
    for (int S : {1, 63, 64, 65, 4096}) std::printf("launches %d %d\n", S, warp_launches(S));

    // counts at frames * 65536 one below, at and one above a multiple of step, and step at both ends of its range
    for (uint32_t step : {WARP_STEP_MIN, 52429u, 65535u, 65536u, 65537u, 78643u, WARP_STEP_MAX})
        for (int32_t frames : {1, 2, 3, 39, 40, 1000, 65535, 65536, 65537, 2147483647})
            std::printf("count %d %u %lld\n", frames, step, (long long)warp_count(frames, step));
    // frames * 65536 = m * step + d for d = -1, 0, 1 cannot be hit by `frames` alone for every step: walk the steps around the divisors
    for (int32_t frames : {3, 17, 1000})
        for (int64_t m : {(int64_t)frames, (int64_t)2 * frames + 1, (int64_t)4 * frames - 1})
            for (int d : {-1, 0, 1}) {
                const int64_t step = ((int64_t)frames << 16) / m + d;
                if (step >= WARP_STEP_MIN && step <= WARP_STEP_MAX) std::printf("count %d %u %lld\n", frames, (uint32_t)step, (long long)warp_count(frames, (uint32_t)step));
            }

    const std::vector<List> lists = {
        {"one", 1, 10, {}, {{0, 0, 10, 0, 65536, 1.f}}},
        {"pauses", 2, 40, {40, 7}, {{0, 0, 0, 5, 0, 0.f}, {0, 20, 20, 0, 65537, 1.f}, {0, 0, 12, 0, 16384, .5f}, {0, 0, 0, 2, 0, 0.f}, {0, 0, 0, 1, 0, 0.f},
                                    {0, 0, 12, 0, 16384, .5f}, {1, 0, 7, 0, 262144, 16.f}, {1, 6, 1, 0, 16384, 0.f}, {1, 0, 0, 130, 0, 0.f}}},
        {"seam", 1, 65, {}, {{0, 2, 63, 0, 65536, 1.f}, {0, 0, 0, 63, 0, 0.f}, {0, 1, 64, 0, 65536, 1.f}, {0, 0, 0, 64, 0, 0.f}, {0, 0, 65, 0, 65536, 1.f},
                             {0, 0, 0, 65, 0, 0.f}, {0, 0, 65, 0, 16384, 1.f}}},
    };
    for (const List& l : lists) show(l, 3);
    {   // a list one longer than a launch carries, and a row whose segments straddle two launches
        List l{"straddle", 3, 40, {40, 40, 39}, {}};
        for (int s = 0; s < WARP_SEGMENTS - 4; ++s) l.seg.push_back({0, s % 38, 1 + s % 3, 0, (uint32_t)(WARP_STEP_MIN + 3001u * (unsigned)s), 1.f});
        for (int s = 0; s < 10; ++s) l.seg.push_back(s % 3 == 1 ? tts_warp_segment_t{1, 0, 0, 1 + s, 0, 0.f} : tts_warp_segment_t{1, 3 * s, 5, 0, 70000, 2.f});
        for (int s = 0; s < 3; ++s) l.seg.push_back({2, 36, 3, 0, 16384, .25f});
        show(l, 0);
        List m{"rows65", 65, 8, {}, {}};
        for (int b = 0; b < 65; ++b) m.seg.push_back({b, 0, 1 + b % 8, 0, 65536, 1.f});
        show(m, 1);
    }

    const List ok = lists[1];
    std::printf("check legal %d\n", answer(ok));
    bad("null", ok, false);
    { List l = ok; l.B = 0; bad("B0", l); }
    { List l = ok; l.T = 0; bad("T0", l); }
    { List l = ok; l.seg.clear(); bad("S0", l); }
    {
        List l{"many", 1, 8, {}, {}};
        for (int s = 0; s < WARP_MAX_SEGMENTS; ++s) l.seg.push_back({0, s % 8, 1, 0, 65536, 1.f});
        std::printf("check legal_max_segments %d\n", answer(l));
        l.seg.push_back({0, 0, 1, 0, 65536, 1.f});
        bad("segments_max", l);
    }
    { List l = ok; l.B = 10; l.n_frames.assign(10, 7); bad("rows_over_segments", l); }
    { List l = ok; l.B = 2147483647; bad("Bmax", l); }   // refused before anything is sized by B
    for (int v : {0, -1, 41}) {
        List l = ok;
        l.n_frames[1] = v;
        std::printf("check n_frames=%d %d\n", v, answer(l));
        std::printf("msg n_frames=%d %s\n", v, g_why.c_str());
    }
    { List l = ok; l.seg[0].row = 1; bad("row_start", l); }
    { List l = ok; l.seg[3].row = 1; bad("row_back", l); }
    { List l = ok; l.B = 3; l.n_frames.push_back(5); l.seg[8].row = 2; l.seg[6].row = 2; bad("row_skip", l); }
    { List l = ok; l.B = 3; l.n_frames.push_back(5); bad("row_end", l); }
    { List l = ok; l.seg[6].row = -1; bad("row_negative", l); }
    { List l = ok; l.seg[2].frames = -1; bad("frames-1", l); }
    { List l = ok; l.seg[3].pause = -2; bad("pause-2", l); }
    { List l = ok; l.seg[2].pause = 3; bad("both", l); }
    { List l = ok; l.seg[4].pause = 0; bad("neither", l); }
    { List l = ok; l.seg[1].first = 21; bad("past_the_row", l); }
    { List l = ok; l.seg[7].first = 7; bad("past_n_frames", l); }      // row 1 holds frames 0 .. 6
    { List l = ok; l.seg[2].first = -1; bad("first-1", l); }
    { List l = ok; l.seg[1].first = 2147483647; bad("first_max", l); }  // (first + frames in 64 bits)
    { List l = ok; l.seg[2].step = WARP_STEP_MIN - 1; bad("step_low", l); }
    { List l = ok; l.seg[2].step = WARP_STEP_MAX + 1; bad("step_high", l); }
    { List l = ok; l.seg[2].step = 0; bad("step0", l); }
    { List l = ok; l.seg[2].step = WARP_STEP_MIN; l.seg[5].step = WARP_STEP_MAX; std::printf("check legal_steps %d\n", answer(l)); }
    { List l = ok; l.seg[6].gain = std::nanf(""); bad("gain_nan", l); }
    { List l = ok; l.seg[6].gain = std::numeric_limits<float>::infinity(); bad("gain_inf", l); }
    { List l = ok; l.seg[6].gain = -1e-30f; bad("gain_negative", l); }
    { List l = ok; l.seg[6].gain = 16.000002f; bad("gain_high", l); }
    { List l = ok; l.seg[6].gain = -0.f; l.seg[7].gain = 16.f; std::printf("check legal_gains %d\n", answer(l)); }
    { List l = ok; l.seg[0].step = 7; l.seg[0].gain = std::nanf(""); l.seg[0].first = -9; std::printf("check legal_pause_fields %d\n", answer(l)); }
    {
        const int64_t n[2] = {5, 9};
        std::printf("msg room %s\n", warp_room(n, 2, 8).c_str());
        std::printf("msg room_max %s\n", warp_room(n, 2, WARP_MAX_T_OUT + 1).c_str());
        expect(warp_room(n, 2, WARP_MAX_T_OUT).empty() && warp_room(n, 2, 9).empty(), "9 .. 2^30 frames are room enough");
        expect((int64_t)WARP_SEGMENTS * (warp_tiles(WARP_MAX_T_OUT) + 1) < ((int64_t)1 << 31), "the largest grid is a legal launch");
    }
    return exit_status();
}
