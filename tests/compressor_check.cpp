// Stand-alone check of the host side of the compressor (csrc/compressor_plan.h compiled as plain C++, no GPU, no library): prints the
// constants, the workspace sizes of a table of lengths, the multiplied-out coefficients, a short row through the five passes with
// its envelope, both chains' states, the designs, the profiles and what tts_compress and tts_set_compressor answer to a list of
// argument sets, for tests/test_compressor_program.py to hold against tests/compressor_oracle.py.  Doubles travel as hex floats.
// Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "compressor_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// known parameters: the coefficients are short binary fractions
static const CmpParams kKnown = {-20.0, 0.25, 6.0, 3.0, 0.875, 0.9375};

static float sample(int i) { return (float)((i * 37) % 101 - 50) / 64.0f * (i % 700 < 350 ? 1.0f : 0.03125f); }

// 0: legal, 1: TTS_ERR_INVALID
static int answer(uintptr_t wav, uintptr_t out, int B, int N, const std::vector<int32_t>* n, const CmpParams* p, uintptr_t env = 0) {
    g_why = compressor_check(wav, out, B, N, n ? n->data() : nullptr, p, env);
    return g_why.empty() ? 0 : 1;
}

int main() {
    std::printf("consts %a %a %a %a %a %a %d\n", CMP_THRESHOLD_MIN, CMP_THRESHOLD_MAX, CMP_KNEE_MAX, CMP_MAKEUP_MIN, CMP_MAKEUP_MAX, CMP_MS_MAX, CMP_UTTS);
    for (int n : {1, 255, 256, 257, 16384, 16385, 275000, 2147483647}) std::printf("ws %d %zu %zu\n", n, cmp_state_doubles(n), cmp_partials(n));

    const CmpCoef k = cmp_coef(kKnown);
    std::printf("coef %a %a %a %a %a\n", k.s1, k.bA, k.AA, k.AR, cmp_power(0.0));
    expect(cmp_power(0.0) == 0.0 && cmp_power(1.0) == 1.0, "the powers of 0 and 1");

    // a row through the five passes: seams, a short last segment, a loud and a quiet stretch
    {
        const int n = 1500;
        std::vector<float> x(n), y(n);
        std::vector<double> env(n);
        for (int i = 0; i < n; ++i) x[i] = sample(i);
        x[700] = std::numeric_limits<float>::quiet_NaN();
        x[701] = std::numeric_limits<float>::infinity();
        x[702] = -0.0f;
        cmp_row(kKnown, x.data(), n, y.data(), env.data());
        for (int i = 0; i < n; ++i) std::printf("row %d %a %a\n", i, (double)y[i], env[i]);
        expect(std::isnan(y[700]) && std::isinf(y[701]) && y[702] == 0.0f && std::signbit(y[702]), "NaN, Inf and -0.0 stay where they are");
        // the chains' states, as cmp_row chains them
        double s = 0.0, t = 0.0;
        for (int i = 0; i + 1 < eq_segments(n); ++i) {
            double c = 0.0, u = 0.0, e1 = s, q = 0.0;
            for (int j = 0; j < EQ_SEG; ++j) cmp_detect(k, (double)x[i * EQ_SEG + j], c, u);
            for (int j = 0; j < EQ_SEG; ++j) cmp_detect(k, (double)x[i * EQ_SEG + j], e1, q);
            std::printf("chain %d %a %a %a %a\n", i, c, s, q, t);
            const double rel = k.AR * s;
            s = c > rel ? c : rel;
            t = k.AA * t + q;
        }
        // slope 1 and make-up 0: the identity
        CmpParams unity = kKnown;
        unity.slope = 1.0, unity.makeup_db = 0.0;
        cmp_row(unity, x.data(), n, y.data(), nullptr);
        for (int i = 0; i < n; ++i)
            if (i != 700) expect(std::memcmp(&x[i], &y[i], 4) == 0, "ratio 1 with make-up 0 is the identity");
    }
    // the gain computer
    for (double L : {-std::numeric_limits<double>::infinity(), -200.0, -23.0, -22.999, -20.0, -17.0, -16.999, 0.0, 60.0}) std::printf("r %a %a\n", L, cmp_reduction(k, L));
    {
        CmpParams hard = kKnown;
        hard.knee_db = 0.0, hard.slope = 0.0;
        const CmpCoef h = cmp_coef(hard);
        for (double L : {-std::numeric_limits<double>::infinity(), -20.0, -19.5, 0.0}) std::printf("rhard %a %a\n", L, cmp_reduction(h, L));
    }

    // designs: 0 legal, 2 TTS_ERR_UNSUPPORTED
    {
        double a = -1.0, r = -1.0;
        const double cases[][3] = {{22050, 5.0, 100.0}, {8000, 0.0, 2000.0}, {192000, 20.0, 0.0}, {48000, 0.01, 10000.0}};
        for (const auto& c : cases) {
            expect(cmp_design((int)c[0], c[1], c[2], &a, &r).empty(), "a design inside the limits");
            std::printf("design %d %a %a %a %a\n", (int)c[0], c[1], c[2], a, r);
            expect(a >= 0.0 && a < 1.0 && r >= 0.0 && r < 1.0, "coefficients in [0, 1)");
        }
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::printf("refuse sr_low %d\n", cmp_design(7999, 5.0, 100.0, &a, &r).empty() ? 0 : 2);
        std::printf("refuse sr_high %d\n", cmp_design(192001, 5.0, 100.0, &a, &r).empty() ? 0 : 2);
        std::printf("refuse attack_negative %d\n", cmp_design(22050, -0.5, 100.0, &a, &r).empty() ? 0 : 2);
        std::printf("refuse attack_nan %d\n", cmp_design(22050, nan, 100.0, &a, &r).empty() ? 0 : 2);
        std::printf("refuse release_long %d\n", cmp_design(22050, 5.0, 10000.5, &a, &r).empty() ? 0 : 2);
        std::printf("refuse legal_zero %d\n", cmp_design(22050, 0.0, 0.0, &a, &r).empty() ? 0 : 2);
        expect(a == 0.0 && r == 0.0, "0 ms gives 0");
    }
    for (int i = 0; i < CMP_PROFILES; ++i)
        for (int sr : {8000, 22050, 192000}) {
            CmpParams p{};
            bool invalid = false;
            expect(cmp_profile(cmp_profiles()[i].name, sr, &p, &invalid).empty() && !invalid, "a profile fits every rate");
            expect(cmp_params_check(p).empty(), "a profile is legal");
            std::printf("profile %s %d %a %a %a %a %a %a\n", cmp_profiles()[i].name, sr, p.threshold_db, p.slope, p.knee_db, p.makeup_db, p.attack_coeff,
                        p.release_coeff);
        }
    {
        CmpParams p{};
        bool invalid = false;
        expect(!cmp_profile("loud", 22050, &p, &invalid).empty() && invalid, "an unknown profile is invalid");
        expect(!cmp_profile(nullptr, 22050, &p, &invalid).empty() && invalid, "a NULL name is invalid");
        expect(!cmp_profile("speech", 7000, &p, &invalid).empty() && !invalid, "a rate outside the limits is unsupported");
    }

    // the argument checks of tts_compress, in the header's order
    const std::vector<int32_t> ls = {5000, 1, 275};
    const uintptr_t W = 0x10000, O = 0x80000, E = 0x100000;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::printf("check legal_ragged %d\n", answer(W, O, 3, 5000, &ls, &kKnown, E));
    std::printf("check legal_in_place %d\n", answer(W, W, 3, 5000, nullptr, &kKnown));
    std::printf("check legal_adjacent %d\n", answer(W, W + 3 * 5000 * 4, 3, 5000, nullptr, &kKnown));
    std::printf("check legal_offset_4 %d\n", answer(W + 4, O + 12, 3, 5000, nullptr, &kKnown, E + 8));
    std::printf("check legal_largest %d\n", answer(W, W, 1, 2147483647, nullptr, &kKnown));
    std::printf("check null_wav %d\n", answer(0, O, 3, 5000, nullptr, &kKnown));
    std::printf("check null_out %d\n", answer(W, 0, 3, 5000, nullptr, &kKnown));
    std::printf("check null_params %d\n", answer(W, O, 3, 5000, nullptr, nullptr));
    std::printf("check B0 %d\n", answer(W, O, 0, 5000, nullptr, &kKnown));
    std::printf("check N0 %d\n", answer(W, O, 3, 0, nullptr, &kKnown));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(W, O, 3, 5000, &l, &kKnown));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }
    struct Edge { const char* name; double CmpParams::*field; double value; };
    const Edge edges[] = {
        {"threshold_above", &CmpParams::threshold_db, 0.25},  {"threshold_below", &CmpParams::threshold_db, -80.25}, {"threshold_nan", &CmpParams::threshold_db, nan},
        {"legal_threshold_0", &CmpParams::threshold_db, 0.0}, {"legal_threshold_min", &CmpParams::threshold_db, -80.0},
        {"slope_above", &CmpParams::slope, 1.25},             {"slope_below", &CmpParams::slope, -0.25},             {"slope_nan", &CmpParams::slope, nan},
        {"legal_slope_0", &CmpParams::slope, 0.0},            {"legal_slope_1", &CmpParams::slope, 1.0},
        {"knee_above", &CmpParams::knee_db, 40.5},            {"knee_below", &CmpParams::knee_db, -0.5},             {"legal_knee_0", &CmpParams::knee_db, 0.0},
        {"legal_knee_40", &CmpParams::knee_db, 40.0},         {"makeup_above", &CmpParams::makeup_db, 24.5},         {"makeup_below", &CmpParams::makeup_db, -24.5},
        {"legal_makeup_24", &CmpParams::makeup_db, 24.0},     {"attack_one", &CmpParams::attack_coeff, 1.0},         {"attack_negative", &CmpParams::attack_coeff, -0.5},
        {"attack_nan", &CmpParams::attack_coeff, nan},        {"legal_attack_0", &CmpParams::attack_coeff, 0.0},     {"release_one", &CmpParams::release_coeff, 1.0},
        {"release_negative", &CmpParams::release_coeff, -0.5}, {"legal_release_0", &CmpParams::release_coeff, 0.0},
    };
    for (const Edge& e : edges) {
        CmpParams p = kKnown;
        p.*(e.field) = e.value;
        std::printf("check %s %d\n", e.name, answer(W, O, 3, 5000, nullptr, &p));
        std::printf("check setting_%s %d\n", e.name, cmp_params_check(p).empty() ? 0 : 1);   // tts_set_compressor asks the parameter checks alone
    }
    std::printf("check misaligned_wav %d\n", answer(W + 2, O, 3, 5000, nullptr, &kKnown));
    std::printf("check misaligned_out %d\n", answer(W, O + 1, 3, 5000, nullptr, &kKnown));
    std::printf("check misaligned_envelope %d\n", answer(W, O, 3, 5000, nullptr, &kKnown, E + 4));
    std::printf("check overlap_ahead %d\n", answer(W, W + 4, 3, 5000, nullptr, &kKnown));
    std::printf("check overlap_behind %d\n", answer(W + 3 * 5000 * 4 - 4, W, 3, 5000, nullptr, &kKnown));
    // the order: an earlier check answers first
    CmpParams bad = kKnown;
    bad.slope = 2.0, bad.threshold_db = 1.0;
    answer(0, O, 0, 5000, nullptr, &bad);
    expect(g_why.find("NULL") != std::string::npos, "NULL pointers first");
    answer(W, O, 0, 5000, nullptr, &bad);
    expect(g_why.find("B, N") != std::string::npos, "then B and N");
    {
        std::vector<int32_t> l = {5000, 0, 275};
        answer(W + 2, O, 3, 5000, &l, &bad);
        expect(g_why.find("n_samples[1]") != std::string::npos, "then the lengths");
    }
    answer(W + 2, W + 6, 3, 5000, nullptr, &bad);
    expect(g_why.find("threshold_db") != std::string::npos, "then the parameters, the threshold first");
    bad.threshold_db = -20.0;
    answer(W + 2, W + 6, 3, 5000, nullptr, &bad);
    expect(g_why.find("slope") != std::string::npos, "then the slope");
    answer(W + 2, W + 6, 3, 5000, nullptr, &kKnown, E + 4);
    expect(g_why.find("wav and out") != std::string::npos, "then the alignment of the rows");
    answer(W, W + 8, 3, 5000, nullptr, &kKnown, E + 4);
    expect(g_why.find("envelope") != std::string::npos, "then the envelope's");
    answer(W, W + 8, 3, 5000, nullptr, &kKnown);
    expect(g_why.find("overlaps") != std::string::npos, "the overlap last");
    return exit_status();
}
