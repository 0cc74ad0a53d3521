// Stand-alone check of the host side of the join (csrc/join_plan.h compiled as plain C++, no GPU, no library): prints the constants,
// the layout -- offsets, fades and group lengths -- of a table of edit lists, the entries the kernel is handed for one of them, and
// what tts_join_plan and tts_join answer to a list of bad argument sets, for tests/test_join_program.py to hold against
// tests/join_oracle.py.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "join_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

struct List {
    const char* name;
    int B, N, fade;
    std::vector<tts_join_piece_t> pieces;
    std::vector<int32_t> group;
};

static std::string g_why;

// 0: legal, 1: TTS_ERR_INVALID
static int answer(const List& l, bool ptrs = true, int G = -1) {
    const int groups = G >= 0 ? G : (l.group.empty() ? 0 : l.group.back() + 1);
    std::vector<int64_t> n_out((size_t)(groups > 0 && groups <= JOIN_MAX_PIECES ? groups : 1));   // (more groups than pieces: refused before a length is written)
    g_why = join_plan(ptrs ? l.pieces.data() : nullptr, (int)l.pieces.size(), l.group.data(), groups, l.B, l.N, l.fade, n_out.data());
    return g_why.empty() ? 0 : 1;
}

static void bad(const char* name, const List& l, bool ptrs = true, int G = -1) {
    std::printf("check %s %d\n", name, answer(l, ptrs, G));
    std::printf("msg %s %s\n", name, g_why.c_str());
}

int main() {
    std::printf("consts %d %d %d %d %d\n", JOIN_PIECES, JOIN_MAX_PIECES, JOIN_MAX_FADE, JOIN_THREADS, JOIN_TILE);
    expect(sizeof(tts_join_piece_t) == 16, "a piece is four int32");
    expect(sizeof(JoinEntry) == 24 && sizeof(JoinChunk) <= 3800, "a launch's entries fit the kernel's argument space");
    for (int P : {1, 127, 128, 129, 4096}) std::printf("launches %d %d\n", P, join_launches(P));

    const std::vector<List> lists = {
        {"one", 1, 10, 0, {{0, 0, 10, 0}}, {0}},
        {"last_gap_ignored", 2, 100, 4, {{1, 3, 20, 7}, {0, 0, 9, -1000}}, {0, 0}},
        {"crossfade", 3, 2003, 64, {{2, 1, 300, -64}, {0, 7, 129, -3}, {2, 1, 7, 0}, {1, 1000, 1003, 5000}, {1, 0, 1, 0}}, {0, 0, 0, 0, 0}},
        {"groups", 5, 2003, 7, {{4, 11, 13, -6}, {3, 0, 14, 2}, {0, 5, 1, 0}, {4, 11, 13, -1}, {1, 2, 2, 1}, {2, 1, 3, 9}}, {0, 0, 1, 2, 2, 2}},
        {"short_fades", 1, 50, 64, {{0, 0, 1, 0}, {0, 1, 2, -1}, {0, 3, 3, -1}, {0, 6, 44, 0}}, {0, 0, 0, 0}},
        {"large_gap", 1, 4, 0, {{0, 0, 4, 2147483647}, {0, 0, 4, 2147483647}, {0, 0, 4, 0}}, {0, 0, 0}},
    };
    for (const List& l : lists) {
        const int P = (int)l.pieces.size(), G = l.group.back() + 1;
        std::vector<int64_t> n_out((size_t)G), off((size_t)P);
        std::vector<int32_t> f((size_t)P);
        const std::string why = join_plan(l.pieces.data(), P, l.group.data(), G, l.B, l.N, l.fade, n_out.data(), off.data(), f.data());
        expect(why.empty(), l.name);
        std::printf("list %s %d %d %d %d %d\n", l.name, l.B, l.N, l.fade, P, G);
        for (int p = 0; p < P; ++p)
            std::printf("piece %s %d %d %d %d %d %d %lld %d\n", l.name, p, l.pieces[p].row, l.pieces[p].first, l.pieces[p].count, l.pieces[p].gap, l.group[p],
                        (long long)off[p], f[p]);
        for (int g = 0; g < G; ++g) std::printf("n_out %s %d %lld\n", l.name, g, (long long)n_out[g]);
        if (std::string(l.name) == "groups") {   // what the kernel is handed: flat starts, and the overlap with the predecessor
            std::vector<JoinEntry> e;
            join_entries(l.pieces.data(), P, l.group.data(), 40, off.data(), e);
            expect((int)e.size() == P + 1, "one entry per piece behind the unused one");
            for (int p = 0; p < P; ++p) std::printf("entry %d %lld %d\n", p, (long long)e[(size_t)p + 1].start, e[(size_t)p + 1].over);
        }
        std::printf("room %s %d %d\n", l.name, join_room(n_out.data(), G, (int)(n_out[0] > 2000000000 ? 2147483647 : n_out[0])).empty() ? 0 : 1,
                    join_room(n_out.data(), G, 0).empty() ? 0 : 1);
    }
    {
        const int64_t n[2] = {5, 9};
        std::printf("msg room %s\n", join_room(n, 2, 8).c_str());
        // a launch's grid times its workgroup stays below 2^32: 2^33 output samples at the most
        const int64_t one[4] = {1, 1, 1, 1};
        std::printf("msg samples %s\n", join_room(one, 4, 2147483647).c_str());
        expect(join_room(one, 4, 2147483647).empty(), "4 * (2^31 - 1) samples fit");
        const int64_t five[5] = {1, 1, 1, 1, 1};
        std::printf("msg samples5 %s\n", join_room(five, 5, 2147483647).c_str());
        expect((JOIN_MAX_SAMPLES / JOIN_TILE + 2) * JOIN_THREADS < ((int64_t)1 << 32), "the largest grid is a legal launch");
    }

    const List ok = lists[3];
    std::printf("check legal %d\n", answer(ok));
    bad("null", ok, false);
    { List l = ok; l.B = 0; bad("B0", l); }
    { List l = ok; l.N = 0; bad("N0", l); }
    { List l = ok; l.pieces.clear(); l.group.clear(); bad("P0", l, true, 1); }
    bad("G0", ok, true, 0);
    bad("G7", ok, true, 7);                  // more groups than pieces: before anything is sized by G
    bad("Gmax", ok, true, 2147483647);
    { List l = ok; l.fade = -1; bad("fade-1", l); }
    { List l = ok; l.fade = JOIN_MAX_FADE; std::printf("check legal_max_fade %d\n", answer(l)); }
    { List l = ok; l.fade = JOIN_MAX_FADE + 1; bad("fade_max", l); }
    {
        List l{"many", 1, 8, 0, {}, {}};
        for (int p = 0; p < JOIN_MAX_PIECES; ++p) l.pieces.push_back({0, p % 8, 1, 0}), l.group.push_back(0);
        std::printf("check legal_max_pieces %d\n", answer(l));
        l.pieces.push_back({0, 0, 1, 0}), l.group.push_back(0);
        bad("pieces_max", l);
    }
    for (int r : {-1, 5}) { List l = ok; l.pieces[2].row = r; bad(r < 0 ? "row-1" : "row5", l); }
    for (int v : {-1, 2003}) { List l = ok; l.pieces[1].first = v; bad(v < 0 ? "first-1" : "first2003", l); }
    for (int v : {0, -1, 1993}) {   // row 4 from 11 on: 1992 samples are left
        List l = ok;
        l.pieces[3].count = v;
        std::printf("check count=%d %d\n", v, answer(l));
        std::printf("msg count=%d %s\n", v, g_why.c_str());
    }
    { List l = ok; l.pieces[3].count = 1992; l.pieces[3].gap = 0; std::printf("check legal_count %d\n", answer(l)); }
    { List l = ok; l.group[0] = 1; bad("group_start", l); }
    { List l = ok; l.group = {0, 0, 1, 0, 0, 0}; bad("group_back", l); }
    { List l = ok; l.group = {0, 0, 2, 2, 2, 2}; bad("group_skip", l); }
    bad("group_end", ok, true, 4);
    { List l = ok; l.pieces[0].gap = -7; bad("gap", l); }        // f = min(7, 13 / 2) = 6
    { List l = ok; l.pieces[3].gap = -2; bad("gap_short", l); }  // the next piece has 2 samples: f = 1
    { List l = ok; l.pieces[2].gap = -5; std::printf("check legal_last_gap %d\n", answer(l)); }   // (a group's last gap is not looked at)
    return exit_status();
}
