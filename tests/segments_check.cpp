// Stand-alone check of what the segment-wise stages share (csrc/segments.h compiled as plain C++, no GPU, no library): holds
// segment_find -- the bisection every kernel of these stages runs -- against a linear scan for every tile of a table of launches,
// prints the tables and what it found, the cut of a list into padded chunks, and the shared refusals for a toy record, for
// tests/test_segments_program.py.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "segments.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

struct ToySegment {
    int32_t row, length;
};
struct ToyEntry {
    int32_t id, tile0, tiles;
};
constexpr ToyEntry TOY_PAD{-1, 0, 0};

// the entries of a list whose segment s owns own[s] tiles, with every launch's numbering
static std::vector<ToyEntry> entries_of(const std::vector<int>& own, std::vector<int64_t>& tiles) {
    std::vector<ToyEntry> e;
    tiles.assign((size_t)segment_launches((int)own.size()), 0);
    for (int s = 0; s < (int)own.size(); ++s) e.push_back({s, segment_take_tiles(tiles, s, own[(size_t)s]), own[(size_t)s]});
    return e;
}

// every tile of every launch of the list: what segment_find answers, against a linear scan for the entry that owns the tile
static void table(const char* name, const std::vector<int>& own) {
    std::vector<int64_t> tiles;
    const std::vector<ToyEntry> e = entries_of(own, tiles);
    expect((int)tiles.size() == segment_launches((int)own.size()), "a tile count per launch");
    int launches = 0;
    const int rc = for_each_segment_launch(e, TOY_PAD, [&](const SegmentChunk<ToyEntry>& c, int n, int l) -> int {
        expect(l == launches++, "the launches come in order");
        expect(n == (l + 1 < (int)tiles.size() ? SEGMENTS_PER_LAUNCH : (int)own.size() - l * SEGMENTS_PER_LAUNCH), "the entries of a launch");
        std::printf("launch %s %d %d %lld", name, l, n, (long long)tiles[(size_t)l]);
        for (int q = 0; q < n; ++q) std::printf(" %d", c.e[q].tiles);
        std::printf("\n");
        for (int q = 0; q < SEGMENTS_PER_LAUNCH; ++q)
            expect(q < n ? c.e[q].id == l * SEGMENTS_PER_LAUNCH + q : c.e[q].id == -1 && c.e[q].tiles == 0, "a chunk is its entries, and the pad behind them");
        for (int tile = 0; tile < (int)tiles[(size_t)l]; ++tile) {
            int scan = -1;
            for (int q = 0; q < n; ++q)
                if (c.e[q].tile0 <= tile && tile < c.e[q].tile0 + c.e[q].tiles) {
                    expect(scan < 0, "one owner per tile");
                    scan = q;
                }
            const int got = segment_find(c.e, n, tile);
            expect(scan >= 0 && got == scan, "segment_find is the linear scan");
            expect(got >= 0 && got < n && c.e[got].tile0 <= tile && tile < c.e[got].tile0 + c.e[got].tiles, "the entry found owns the tile");
            std::printf("own %s %d %d %d\n", name, l, tile, got);
        }
        return 0;
    });
    expect(rc == 0 && launches == (int)tiles.size(), "every launch is visited");
}

static std::vector<int> pattern(int n, int (*f)(int)) {
    std::vector<int> own;
    for (int s = 0; s < n; ++s) own.push_back(f(s));
    return own;
}

static void refusal(const char* name, const std::vector<ToySegment>& seg, int B, const std::vector<int32_t>& len, int W) {
    const std::string why = segment_rows_refusal(seg.data(), (int)seg.size(), B, "toy_max_segments()", "n_toy", len.empty() ? nullptr : len.data(), "W", W);
    std::printf("check %s %d\n", name, why.empty() ? 0 : 1);
    std::printf("msg %s %s\n", name, why.c_str());
}

int main() {
    std::printf("consts %d %d\n", SEGMENTS_PER_LAUNCH, MAX_SEGMENTS);
    for (int S : {1, 63, 64, 65, 4096}) std::printf("launches %d %d\n", S, segment_launches(S));
    expect(sizeof(SegmentChunk<ToyEntry>) == SEGMENTS_PER_LAUNCH * sizeof(ToyEntry), "a chunk is its entries and nothing else");

    table("one", {3});
    table("two", {2, 1});
    table("two_first_empty", {0, 4});
    table("two_last_empty", {4, 0});
    table("runs", {2, 0, 0, 0, 3, 0, 0, 1, 0, 0});
    table("n63", pattern(63, [](int s) { return s % 4; }));                            // the first and every fourth own nothing
    table("n63_last_empty", pattern(63, [](int s) { return (62 - s) % 3; }));
    table("n64_ones", pattern(64, [](int) { return 1; }));
    table("n64", pattern(64, [](int s) { return (s * 7 + 3) % 5; }));
    table("n64_first_empty", pattern(64, [](int s) { return s == 0 ? 0 : 1 + s % 2; }));
    table("n64_middle_empty", pattern(64, [](int s) { return s >= 30 && s < 34 ? 0 : 2; }));   // a run over the bisection's first probe
    table("n64_last_empty", pattern(64, [](int s) { return s == 63 ? 0 : 1; }));
    table("n64_only_first", pattern(64, [](int s) { return s == 0 ? 5 : 0; }));
    table("n64_only_17", pattern(64, [](int s) { return s == 17 ? 5 : 0; }));
    table("n64_only_last", pattern(64, [](int s) { return s == 63 ? 5 : 0; }));
    table("n130", pattern(130, [](int s) { return s % 3 == 1 ? 0 : 1 + s % 4; }));       // three launches, each numbered from 0

    const std::vector<ToySegment> ok = {{0, 5}, {0, 1}, {0, 2}, {1, 7}, {1, 7}, {2, 1}};
    const std::vector<int32_t> len = {40, 7, 1};
    refusal("legal", ok, 3, len, 40);
    refusal("legal_no_lengths", ok, 3, {}, 40);
    {
        std::vector<ToySegment> many((size_t)MAX_SEGMENTS, ToySegment{0, 1});
        refusal("legal_max_segments", many, 1, {}, 40);
        many.push_back({0, 1});
        refusal("segments_max", many, 1, {}, 40);
    }
    refusal("rows_over_segments", ok, 7, {}, 40);
    refusal("length", ok, 3, {40, 41, 1}, 40);
    { auto l = ok; l[0].row = 1; refusal("row_start", l, 3, len, 40); }
    { auto l = ok; l[4].row = 0; refusal("row_back", l, 3, len, 40); }
    { auto l = ok; l[3].row = l[4].row = 2; refusal("row_skip", l, 3, len, 40); }
    { auto l = ok; l[2].row = -1; refusal("row_negative", l, 3, len, 40); }
    { auto l = ok; l[5].row = 1; refusal("row_end", l, 3, len, 40); }
    {
        const int64_t n[2] = {5, 9};
        std::printf("msg room %s\n", segment_room("W_out", n, 2, 8, 1 << 30).c_str());
        std::printf("msg room_max %s\n", segment_room("W_out", n, 2, (1 << 30) + 1, 1 << 30).c_str());
        expect(segment_room("W_out", n, 2, 9, 1 << 30).empty() && segment_room("W_out", n, 2, 1 << 30, 1 << 30).empty(), "9 .. 2^30 are room enough");
    }
    return exit_status();
}
