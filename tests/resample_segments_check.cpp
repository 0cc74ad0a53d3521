// Stand-alone check of the host side of the segment-wise resampler (csrc/resample_segments_plan.h compiled as plain C++, no GPU, no
// library): prints the constants, the output samples of every segment and row of a table of segment lists, the cut of each into
// launches and tiles, and what the plan answers to a list of bad argument sets, for tests/test_resample_segments_program.py to hold
// against tests/resample_segments_oracle.py.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "resample_segments_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

struct List {
    const char* name;
    int B, n;
    std::vector<int32_t> n_samples;   // empty: all n
    std::vector<tts_resample_segment_t> seg;
};

static std::string g_why;

// 0: legal, 1: TTS_ERR_INVALID
static int answer(const List& l, bool ptrs = true) {
    std::vector<int64_t> n_out((size_t)(l.B > 0 && l.B <= RSEG_MAX_SEGMENTS ? l.B : 1));   // (more rows than segments: refused before a length is written)
    g_why = resample_segments_plan(ptrs ? l.seg.data() : nullptr, (int)l.seg.size(), l.B, l.n, l.n_samples.empty() ? nullptr : l.n_samples.data(),
                                   n_out.data());
    return g_why.empty() ? 0 : 1;
}

static void bad(const char* name, const List& l, bool ptrs = true) {
    std::printf("check %s %d\n", name, answer(l, ptrs));
    std::printf("msg %s %s\n", name, g_why.c_str());
}

// the list, its lengths and its cut at N_out = the longest row + extra
static void show(const List& l, int extra) {
    const int S = (int)l.seg.size();
    std::vector<int64_t> n_out((size_t)l.B), count((size_t)S);
    const int32_t* ns = l.n_samples.empty() ? nullptr : l.n_samples.data();
    const std::string why = resample_segments_plan(l.seg.data(), S, l.B, l.n, ns, n_out.data(), count.data());
    expect(why.empty(), l.name);
    if (!why.empty()) return;
    int64_t longest = 1;
    for (int64_t v : n_out) longest = v > longest ? v : longest;
    const int N_out = (int)longest + extra;
    std::printf("list %s %d %d %d %d\n", l.name, l.B, l.n, S, N_out);
    for (int b = 0; b < l.B; ++b) std::printf("samples %s %d %d\n", l.name, b, ns ? ns[b] : l.n);
    for (int s = 0; s < S; ++s)
        std::printf("seg %s %d %d %d %d %a %lld\n", l.name, s, l.seg[s].row, l.seg[s].first, l.seg[s].samples, l.seg[s].ratio, (long long)count[s]);
    for (int b = 0; b < l.B; ++b) std::printf("n_out %s %d %lld\n", l.name, b, (long long)n_out[b]);
    expect(resample_segments_room(n_out.data(), l.B, N_out).empty(), "the longest row is room enough");
    std::vector<double> below;
    bool above = false;
    resample_segments_ratios(l.seg.data(), S, below, &above);
    expect((int)below.size() <= RSEG_MAX_RATIOS, "a legal list has at most 16 ratios below 1");
    std::printf("ratios %s %d %d\n", l.name, (int)below.size(), above ? 1 : 0);
    std::vector<RsegEntry> e;
    std::vector<int64_t> tiles;
    std::vector<int> lds;
    resample_segments_entries(l.seg.data(), S, l.n, ns, N_out, count.data(), below, e, tiles, lds);
    expect((int)e.size() == S && (int)tiles.size() == rseg_launches(S) && lds.size() == tiles.size(), "an entry per segment, a tile count per launch");
    for (int s = 0; s < S; ++s) {
        const RsegEntry& w = e[(size_t)s];
        std::printf("entry %s %d %d %d %d %d %d %d %d\n", l.name, s, s / RSEG_SEGMENTS, w.tile0, (int)rseg_tiles(w.span), w.o, w.count, w.span, w.tab);
        expect(w.span >= 0 && w.count <= w.span && (int64_t)w.o + w.span <= N_out, "what a segment owns lies inside its row");
        expect(w.first >= 0 && (int64_t)w.first + l.seg[s].samples <= w.n && w.n <= l.n, "a segment's source lies inside its row");
        const bool copy = l.seg[s].ratio == 1.0;
        expect(copy ? w.tab == -1 : l.seg[s].ratio > 1.0 ? w.tab == 0 : (w.tab >= 1 && w.tab <= (int)below.size() && below[(size_t)w.tab - 1] == l.seg[s].ratio),
               "a segment walks its own ratio's table");
        if (!copy) {
            const ResampleConsts c = resample_consts(l.seg[s].ratio);
            expect(w.inc == c.inc && w.scale == c.scale, "inc and scale are the ratio's");
            // the LDS of the launch holds the windows of every tile of the segment: the kernel's own span, tile by tile
            for (int64_t j0 = 0; j0 < w.count; j0 += RSEG_TILE) {
                const int64_t j1 = std::min<int64_t>(j0 + RSEG_TILE - 1, w.count - 1);
                const long long span = (long long)((double)j1 * c.inc) - (long long)((double)j0 * c.inc) + 2 * c.taps_max;
                expect(span <= lds[(size_t)(s / RSEG_SEGMENTS)], "a tile's window fits the launch's LDS");
            }
        }
    }
    for (size_t k = 0; k < tiles.size(); ++k) std::printf("tiles %s %d %lld %d\n", l.name, (int)k, (long long)tiles[k], lds[k]);
}

int main() {
    const double down4 = std::exp2(-4.0 / 12.0), up3 = std::exp2(3.0 / 12.0);
    std::printf("consts %d %d %d %d\n", RSEG_SEGMENTS, RSEG_MAX_SEGMENTS, RSEG_MAX_RATIOS, RSEG_TILE);
    expect(sizeof(tts_resample_segment_t) == 24, "a segment is four int32 and a double");
    expect(sizeof(RsegEntry) == 48 && sizeof(RsegChunk) + 8 * (RSEG_MAX_RATIOS + 1) + 64 <= 3800, "a launch's entries and tables fit the kernel's argument space");
    for (int S : {1, 63, 64, 65, 4096}) std::printf("launches %d %d\n", S, rseg_launches(S));
    for (double ratio : {0.25, 0.5, down4, 16000.0 / 22050.0, 1.0, up3, 2.0, 4.0})
        for (int32_t samples : {1, 2, 3, 63, 64, 700, 5000, 2147483647}) std::printf("count %d %a %lld\n", samples, ratio, (long long)rseg_count(samples, ratio));
    for (double ratio : {0.25, down4, 1.5, 4.0}) std::printf("span_max %a %d\n", ratio, rseg_span_max(resample_consts(ratio)));

    const std::vector<List> lists = {
        {"one", 1, 10, {}, {{0, 0, 10, 0, 2.0}}},
        {"mixed", 3, 700, {700, 64, 1},
         {{0, 100, 255, 0, 1.0}, {0, 188, 512, 0, 0.5}, {0, 186, 514, 0, 0.5}, {0, 130, 510, 0, 0.5}, {0, 300, 1, 0, 0.25}, {0, 0, 700, 0, down4},
          {1, 0, 64, 0, 4.0}, {1, 32, 32, 0, up3}, {1, 0, 1, 0, 0.5}, {2, 0, 1, 0, 0.25}}},
    };
    for (const List& l : lists) show(l, 3);
    {   // a list one longer than a launch carries; rows whose segments straddle two launches; a row that produces nothing
        List l{"straddle", 3, 400, {400, 400, 399}, {}};
        for (int s = 0; s < RSEG_SEGMENTS - 4; ++s) l.seg.push_back({0, s % 380, 1 + s % 19, 0, s % 5 == 0 ? 1.0 : 0.3 + 0.04 * (s % 16)});
        for (int s = 0; s < 10; ++s) l.seg.push_back({1, 30 * s, 100, 0, s % 3 == 1 ? 1.0 : 3.5});
        for (int s = 0; s < 3; ++s) l.seg.push_back({2, 396, 3, 0, 0.3});
        show(l, 0);
        List m{"rows65", 65, 8, {}, {}};
        for (int b = 0; b < 65; ++b) m.seg.push_back({b, 0, 1 + b % 8, 0, b % 2 ? 2.0 : 1.0});
        show(m, 1);
    }

    const List ok = lists[1];
    std::printf("check legal %d\n", answer(ok));
    bad("null", ok, false);
    { List l = ok; l.B = 0; bad("B0", l); }
    { List l = ok; l.n = 0; bad("n0", l); }
    { List l = ok; l.seg.clear(); bad("S0", l); }
    {
        List l{"many", 1, 8, {}, {}};
        for (int s = 0; s < RSEG_MAX_SEGMENTS; ++s) l.seg.push_back({0, s % 8, 1, 0, 1.0});
        std::printf("check legal_max_segments %d\n", answer(l));
        l.seg.push_back({0, 0, 1, 0, 1.0});
        bad("segments_max", l);
    }
    { List l = ok; l.B = 11; l.n_samples.assign(11, 7); bad("rows_over_segments", l); }
    { List l = ok; l.B = 2147483647; bad("Bmax", l); }   // refused before anything is sized by B
    for (int v : {0, -1, 701}) {
        List l = ok;
        l.n_samples[1] = v;
        std::printf("check n_samples=%d %d\n", v, answer(l));
        std::printf("msg n_samples=%d %s\n", v, g_why.c_str());
    }
    { List l = ok; l.seg[0].row = 1; bad("row_start", l); }
    { List l = ok; l.seg[7].row = 0; bad("row_back", l); }
    { List l = ok; for (int s = 6; s < 9; ++s) l.seg[s].row = 2; bad("row_skip", l); }
    { List l = ok; l.B = 4; l.n_samples.push_back(5); bad("row_end", l); }
    { List l = ok; l.seg[6].row = -1; bad("row_negative", l); }
    { List l = ok; l.seg[2].samples = 0; bad("samples0", l); }
    { List l = ok; l.seg[2].samples = -3; bad("samples-3", l); }
    { List l = ok; l.seg[1].first = 189; bad("past_the_row", l); }
    { List l = ok; l.seg[7].first = 33; bad("past_n_samples", l); }      // row 1 holds samples 0 .. 63
    { List l = ok; l.seg[2].first = -1; bad("first-1", l); }
    { List l = ok; l.seg[1].first = 2147483647; bad("first_max", l); }   // (first + samples in 64 bits)
    { List l = ok; l.seg[3].ratio = 0.2499999; bad("ratio_low", l); }
    { List l = ok; l.seg[3].ratio = 4.0000001; bad("ratio_high", l); }
    { List l = ok; l.seg[3].ratio = std::nan(""); bad("ratio_nan", l); }
    { List l = ok; l.seg[3].ratio = std::numeric_limits<double>::infinity(); bad("ratio_inf", l); }
    { List l = ok; l.seg[3].ratio = -1.0; bad("ratio_negative", l); }
    { List l = ok; l.seg[3].ratio = 0.25; l.seg[6].ratio = 4.0; std::printf("check legal_ratios %d\n", answer(l)); }
    { List l = ok; l.seg[4].reserved = 1; bad("reserved", l); }
    { List l = ok; l.seg[4].reserved = 1; l.seg[3].ratio = 9.0; bad("ratio_before_reserved", l); }
    {
        List l{"sixteen", 1, 100, {}, {}};
        for (int k = 0; k < RSEG_MAX_RATIOS; ++k) l.seg.push_back({0, k, 10, 0, std::exp2(-(k + 1) / 48.0)});
        l.seg.push_back({0, 0, 10, 0, l.seg[3].ratio});
        l.seg.push_back({0, 0, 10, 0, 1.75});
        l.seg.push_back({0, 0, 10, 0, 1.0});
        std::printf("check legal_sixteen_ratios %d\n", answer(l));
        l.seg.push_back({0, 0, 10, 0, 0.3});
        l.seg.push_back({0, 0, 10, 0, 0.31});
        bad("ratios_max", l);
        l.seg[20].reserved = 5;
        bad("reserved_before_ratios_max", l);
    }
    {
        const int64_t n[2] = {5, 9};
        std::printf("msg room %s\n", resample_segments_room(n, 2, 8).c_str());
        std::printf("msg room_max %s\n", resample_segments_room(n, 2, RSEG_MAX_N_OUT + 1).c_str());
        expect(resample_segments_room(n, 2, RSEG_MAX_N_OUT).empty() && resample_segments_room(n, 2, 9).empty(), "9 .. 2^30 samples are room enough");
        expect((int64_t)RSEG_SEGMENTS * (rseg_tiles(RSEG_MAX_N_OUT) + 1) < ((int64_t)1 << 31), "the largest grid is a legal launch");
    }
    return exit_status();
}
