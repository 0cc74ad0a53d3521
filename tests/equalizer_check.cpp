// Stand-alone check of the host side of the equaliser (csrc/equalizer_plan.h compiled as plain C++, no GPU, no library): prints the
// constants, the cut of a table of lengths, the workspace sizes, the transition of a known cascade, a segment's end state, a short
// row through the three passes, a table of designs and what tts_equalize and tts_set_equalizer answer to a list of argument sets, for
// tests/test_equalizer_program.py to hold against tests/equalizer_oracle.py.  Doubles travel as hex floats.  Built with
// -fsanitize=address,undefined where the compiler has the runtimes.
#include "equalizer_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// a known cascade: every coefficient is a short binary fraction
static const double kKnown[15] = {0.5, 0.25, -0.125, -0.5, 0.25, 1.0, -2.0, 1.0, -1.5, 0.5625, 0.75, 0.0, -0.75, 0.25, -0.5};

static float sample(int i) { return (float)((i * 37) % 101 - 50) / 64.0f; }

// 0: legal, 1: TTS_ERR_INVALID
static int answer(uintptr_t wav, uintptr_t out, int B, int N, const std::vector<int32_t>* n, const double* sos, int S) {
    g_why = equalizer_check(wav, out, B, N, n ? n->data() : nullptr, sos, S);
    return g_why.empty() ? 0 : 1;
}

int main() {
    std::printf("consts %d %d %d %d %d %d %a %a %a %a %a %a %zu %d\n", EQ_MAX_SECTIONS, EQ_SEG, EQ_TILE_SEGS, EQ_UTTS, EQ_SR_MIN, EQ_SR_MAX, EQ_F_MIN,
                EQ_F_MAX, EQ_Q_MIN, EQ_Q_MAX, EQ_GAIN_MIN, EQ_GAIN_MAX, eq_lds_bytes(), EQ_LDS_STRIDE);
    expect(EQ_TILE == EQ_TILE_SEGS * EQ_SEG && (EQ_SEG & (EQ_SEG - 1)) == 0, "a tile is whole segments, a segment a power of two");
    expect(EQ_LDS_STRIDE % 32 == 1, "the lanes of a step hit different banks");

    for (int n : {1, 255, 256, 257, 16383, 16384, 16385, 275000, 2147483647}) {
        const long long segs = eq_segments(n);
        std::printf("cut %d %lld %d %lld\n", n, segs, eq_segment_len(n, segs - 1), eq_tiles(n));
        long long total = 0;
        for (long long i = std::max(0LL, segs - 3); i < segs; ++i) total += eq_segment_len(n, i);
        expect(total == n - std::max(0LL, segs - 3) * EQ_SEG, "the segments cover the row");
        expect(eq_segment_len(n, segs - 1) >= 1 && eq_segment_len(n, segs - 1) <= EQ_SEG, "the last segment holds 1 .. EQ_SEG samples");
        expect(eq_tiles(n) * EQ_TILE_SEGS >= segs && (eq_tiles(n) - 1) * EQ_TILE_SEGS < segs, "the tiles cover the segments");
        for (int S : {1, 5, 8}) std::printf("ws %d %d %zu %zu\n", n, S, eq_state_doubles(n, S), eq_transition_doubles(S));
    }

    // the transition of the known cascade, and that it IS the recurrence on zero input
    {
        double M[36];
        eq_transition(kKnown, 3, M);
        for (int r = 0; r < 6; ++r)
            for (int j = 0; j < 6; ++j) std::printf("M %d %d %a\n", r, j, M[6 * r + j]);
        double st[6] = {0.25, -0.5, 1.0, 2.0, -0.125, 0.75}, S[6] = {0.25, -0.5, 1.0, 2.0, -0.125, 0.75};
        const double zero[6] = {};
        for (int i = 0; i < EQ_SEG; ++i) eq_sample(kKnown, 3, st, 0.0);
        eq_chain(M, 3, zero, S);
        for (int r = 0; r < 6; ++r) expect(std::fabs(S[r] - st[r]) <= 1e-12 * (1.0 + std::fabs(st[r])), "the transition is the recurrence");
        expect(M[6 * 0 + 2] == 0.0 && M[6 * 1 + 4] == 0.0 && M[6 * 3 + 5] == 0.0, "a section's state does not depend on a later one's");
    }
    // a segment's end state from the zero state
    {
        double st[6] = {};
        for (int i = 0; i < EQ_SEG; ++i) eq_sample(kKnown, 3, st, (double)sample(i));
        for (int r = 0; r < 6; ++r) std::printf("end %d %a\n", r, st[r]);
    }
    // a short row through the three passes: two seams and a short last segment
    {
        const int n = 600;
        std::vector<float> x(n), y(n);
        for (int i = 0; i < n; ++i) x[i] = sample(i);
        eq_filter_row(kKnown, 3, x.data(), n, y.data());
        for (int i = 0; i < n; ++i) std::printf("row %d %a\n", i, (double)y[i]);
    }

    // designs
    {
        double sos[5];
        bool invalid = false;
        const double cases[][5] = {{EQ_LOWPASS, 22050, 3400.0, EQ_Q_BUTTER4[0], 0.0}, {EQ_HIGHPASS, 192000, 20.0, EQ_Q_BUTTER2, 0.0},
                                   {EQ_PEAK, 48000, 3000.0, 1.0, 3.0},                {EQ_PEAK, 8000, EQ_F_MIN * 8000.0, 30.0, -40.0},
                                   {EQ_LOWSHELF, 22050, 200.0, EQ_Q_BUTTER2, 2.0},    {EQ_HIGHSHELF, 44100, 6000.0, 0.1, 24.0},
                                   {EQ_LOWPASS, 8000, EQ_F_MAX * 8000.0, 0.5, 0.0}};
        for (const auto& c : cases) {
            const std::string why = eq_design((int)c[0], (int)c[1], c[2], c[3], c[4], sos, &invalid);
            expect(why.empty() && !invalid, "a design inside the limits");
            std::printf("design %d %d %a %a %a %a %a %a %a %a\n", (int)c[0], (int)c[1], c[2], c[3], c[4], sos[0], sos[1], sos[2], sos[3], sos[4]);
            expect(eq_sections_check(sos, 1).empty(), "a design is stable");
        }
        // 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
        auto refused = [&](int kind, int sr, double f0, double q, double g) {
            const std::string why = eq_design(kind, sr, f0, q, g, sos, &invalid);
            return why.empty() ? 0 : invalid ? 1 : 2;
        };
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::printf("refuse kind %d\n", refused(5, 22050, 1000.0, 1.0, 0.0));
        std::printf("refuse kind_negative %d\n", refused(-1, 22050, 1000.0, 1.0, 0.0));
        std::printf("refuse sr_low_above %d\n", refused(EQ_PEAK, 7999, 1000.0, 1.0, 0.0));
        std::printf("refuse sr_high_above %d\n", refused(EQ_PEAK, 192001, 1000.0, 1.0, 0.0));
        std::printf("refuse f_low_above %d\n", refused(EQ_HIGHPASS, 22050, 2.0, 1.0, 0.0));
        std::printf("refuse f_high_above %d\n", refused(EQ_LOWPASS, 8000, 3921.0, 1.0, 0.0));
        std::printf("refuse f_nan_above %d\n", refused(EQ_LOWPASS, 8000, nan, 1.0, 0.0));
        std::printf("refuse q_low_above %d\n", refused(EQ_LOWPASS, 22050, 1000.0, 0.09, 0.0));
        std::printf("refuse q_high_above %d\n", refused(EQ_LOWPASS, 22050, 1000.0, 30.5, 0.0));
        std::printf("refuse q_nan_above %d\n", refused(EQ_LOWPASS, 22050, 1000.0, nan, 0.0));
        std::printf("refuse gain_low_above %d\n", refused(EQ_PEAK, 22050, 1000.0, 1.0, -40.5));
        std::printf("refuse gain_high_above %d\n", refused(EQ_HIGHSHELF, 22050, 1000.0, 1.0, 24.5));
        std::printf("refuse gain_nan_above %d\n", refused(EQ_LOWSHELF, 22050, 1000.0, 1.0, nan));
        std::printf("refuse legal_gain_unread %d\n", refused(EQ_LOWPASS, 22050, 1000.0, 1.0, nan));
    }
    // profiles
    for (int p = 0; p < EQ_PROFILES; ++p)
        for (int sr : {8000, 22050, 48000}) {
            double sos[5 * EQ_MAX_SECTIONS];
            int n = 0;
            bool invalid = false;
            const std::string why = eq_profile(eq_profiles()[p].name, sr, sos, &n, &invalid);
            std::printf("profile %s %d %d %d\n", eq_profiles()[p].name, sr, why.empty() ? 0 : invalid ? 1 : 2, n);
            expect(why.empty() || why.find(eq_profiles()[p].name) != std::string::npos, "a refusal names the profile");
        }
    {
        double sos[5 * EQ_MAX_SECTIONS];
        int n = 0;
        bool invalid = false;
        expect(!eq_profile("loud", 22050, sos, &n, &invalid).empty() && invalid, "an unknown profile is invalid");
        expect(!eq_profile(nullptr, 22050, sos, &n, &invalid).empty() && invalid, "a NULL name is invalid");
    }

    // the argument checks of tts_equalize, in the header's order
    const std::vector<int32_t> ls = {5000, 1, 275};
    const uintptr_t W = 0x10000, O = 0x80000;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double eight[40];
    for (int s = 0; s < 8; ++s)
        for (int c = 0; c < 5; ++c) eight[5 * s + c] = kKnown[c];
    std::printf("check legal_ragged %d\n", answer(W, O, 3, 5000, &ls, kKnown, 3));
    std::printf("check legal_in_place %d\n", answer(W, W, 3, 5000, nullptr, kKnown, 1));
    std::printf("check legal_eight %d\n", answer(W, O, 1, 1, nullptr, eight, 8));
    std::printf("check legal_adjacent %d\n", answer(W, W + 3 * 5000 * 4, 3, 5000, nullptr, kKnown, 3));
    std::printf("check legal_offset_4 %d\n", answer(W + 4, O + 12, 3, 5000, nullptr, kKnown, 3));
    std::printf("check legal_largest %d\n", answer(W, W, 1, 2147483647, nullptr, kKnown, 3));
    std::printf("check null_wav %d\n", answer(0, O, 3, 5000, nullptr, kKnown, 3));
    std::printf("check null_out %d\n", answer(W, 0, 3, 5000, nullptr, kKnown, 3));
    std::printf("check null_sos %d\n", answer(W, O, 3, 5000, nullptr, nullptr, 3));
    std::printf("check B0 %d\n", answer(W, O, 0, 5000, nullptr, kKnown, 3));
    std::printf("check N0 %d\n", answer(W, O, 3, 0, nullptr, kKnown, 3));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(W, O, 3, 5000, &l, kKnown, 3));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }
    std::printf("check sections0 %d\n", answer(W, O, 3, 5000, nullptr, kKnown, 0));
    std::printf("check sections9 %d\n", answer(W, O, 3, 5000, nullptr, eight, 9));
    for (double v : {nan, inf, -inf}) {
        double k[15];
        for (int i = 0; i < 15; ++i) k[i] = kKnown[i];
        k[7] = v;
        std::printf("check coefficient_%s %d\n", std::isnan(v) ? "nan" : v > 0 ? "inf" : "minus_inf", answer(W, O, 3, 5000, nullptr, k, 3));
    }
    const double unstable[][2] = {{0.0, 1.0}, {0.0, -1.0}, {1.5, 0.5}, {-1.5, 0.5}, {2.0, 1.0}, {0.0, 1.5}, {-2.5, 0.9}};
    int u = 0;
    for (const auto& a : unstable) {
        double k[5] = {1.0, 0.0, 0.0, a[0], a[1]};
        std::printf("check unstable_%d %d\n", u++, answer(W, O, 3, 5000, nullptr, k, 1));
    }
    {
        const double edge[5] = {1.0, 0.0, 0.0, -1.99, 0.9901};   // just inside the triangle
        std::printf("check legal_near_the_edge %d\n", answer(W, O, 3, 5000, nullptr, edge, 1));
    }
    std::printf("check misaligned_wav %d\n", answer(W + 2, O, 3, 5000, nullptr, kKnown, 3));
    std::printf("check misaligned_out %d\n", answer(W, O + 1, 3, 5000, nullptr, kKnown, 3));
    std::printf("check overlap_ahead %d\n", answer(W, W + 4, 3, 5000, nullptr, kKnown, 3));
    std::printf("check overlap_behind %d\n", answer(W + 3 * 5000 * 4 - 4, W, 3, 5000, nullptr, kKnown, 3));
    // the order: an earlier check answers first
    answer(0, O, 0, 5000, nullptr, kKnown, 0);
    expect(g_why.find("NULL") != std::string::npos, "NULL pointers first");
    answer(W, O, 0, 5000, nullptr, kKnown, 0);
    expect(g_why.find("B, N") != std::string::npos, "then B and N");
    {
        std::vector<int32_t> l = {5000, 0, 275};
        answer(W + 2, O, 3, 5000, &l, kKnown, 0);
        expect(g_why.find("n_samples[1]") != std::string::npos, "then the lengths");
    }
    answer(W + 2, W + 6, 3, 5000, nullptr, kKnown, 0);
    expect(g_why.find("n_sections") != std::string::npos, "then the number of sections");
    {
        double k[5] = {nan, 0.0, 0.0, 0.0, 1.5};
        answer(W + 2, W + 6, 3, 5000, nullptr, k, 1);
        expect(g_why.find("not finite") != std::string::npos, "then the coefficients");
        k[0] = 1.0;
        answer(W + 2, W + 6, 3, 5000, nullptr, k, 1);
        expect(g_why.find("not stable") != std::string::npos, "then the stability triangle");
    }
    answer(W + 2, W + 6, 3, 5000, nullptr, kKnown, 3);
    expect(g_why.find("aligned") != std::string::npos, "then the alignment");
    answer(W, W + 8, 3, 5000, nullptr, kKnown, 3);
    expect(g_why.find("overlaps") != std::string::npos, "the overlap last");
    // tts_set_equalizer asks the section checks alone
    std::printf("check legal_setting %d\n", eq_sections_check(kKnown, 3).empty() ? 0 : 1);
    std::printf("check setting_sections9 %d\n", eq_sections_check(eight, 9).empty() ? 0 : 1);
    return exit_status();
}
