// Stand-alone check of the host side of the loudness stage (csrc/loudness_plan.h compiled as plain C++, no GPU, no library): prints
// the cut -- step, segment, segment lengths, steps and blocks -- for a table of sampling rates and lengths, and what tts_loudness,
// tts_loudness_normalize and tts_set_loudness answer to a list of argument sets, for tests/test_loudness_program.py to hold against
// tests/loudness_oracle.py.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "loudness_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// 0: legal, 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
static int answer(bool ptrs, int B, int N, const std::vector<int32_t>* n, int sr, bool normalize, double target, double peak) {
    bool unsupported = false;
    const std::string why = loudness_check(ptrs, B, N, n ? n->data() : nullptr, sr, normalize, target, peak, &unsupported);
    g_why = why;
    expect(why.empty() ? !unsupported : true, "unsupported is set with a reason only");
    return why.empty() ? 0 : unsupported ? 2 : 1;
}

int main() {
    std::printf("consts %d %d %d %d %.17g %.17g\n", LOUD_SR_MIN, LOUD_SR_MAX, LOUD_SEGS, LOUD_UTTS, LOUD_Z_ABS, LOUD_REL);
    expect(64 % LOUD_SEGS == 0, "a round of the chain holds whole steps");

    for (int sr : {8000, 8001, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 176400, 192000}) {
        const int s = loud_step(sr), c = loud_segment(sr);
        std::printf("cut %d %d %d", sr, s, c);
        int total = 0;
        for (int q = 0; q < LOUD_SEGS; ++q) {
            std::printf(" %d", loud_segment_len(sr, q));
            total += loud_segment_len(sr, q);
            expect(loud_segment_len(sr, q) >= 1 && loud_segment_len(sr, q) <= c, "a segment holds 1 .. c samples");
        }
        std::printf("\n");
        expect(total == s, "the segments of a step cover it");
        for (int n : {1, s - 1, 4 * s - 1, 4 * s, 4 * s + 1, 5 * s - 1, 5 * s + 17, 11 * s + c - 1, 11 * s + c, 275000, 2147483647}) {
            std::printf("blocks %d %d %d %d %d %zu\n", sr, n, loud_steps(n, sr), loud_blocks(n, sr), loud_steps_read(n, sr), loud_ws_doubles(n, sr));
            // the last sample a pass reads lies inside the utterance
            expect((long long)loud_steps_read(n, sr) * s <= n, "reads stay inside the utterance");
            expect(loud_blocks(n, sr) == 0 || loud_blocks(n, sr) + 3 == loud_steps_read(n, sr), "a block is four steps");
        }
    }

    // the transition of a segment is the recurrence on zero input: M maps a state to the state len samples later
    {
        const LoudFilter f = loud_filter(22050);
        double M[16];
        loud_transition(f.k, loud_segment(22050), M);
        double st[4] = {0.25, -0.5, 1.0, 2.0}, S[4] = {0.25, -0.5, 1.0, 2.0};
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < loud_segment(22050); ++i) loud_sample(f.k, st, 0.0);
        loud_chain(M, zero, S);
        for (int r = 0; r < 4; ++r) expect(std::fabs(S[r] - st[r]) <= 1e-12 * (1.0 + std::fabs(st[r])), "the transition is the recurrence");
        expect(M[2] == 0.0 && M[3] == 0.0 && M[6] == 0.0 && M[7] == 0.0, "the shelf's state does not depend on the high-pass's");
    }

    const std::vector<int32_t> ls = {5000, 1, 275};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::printf("check legal_ragged %d\n", answer(true, 3, 5000, &ls, 22050, false, 0.0, 1.0));
    std::printf("check legal_uniform %d\n", answer(true, 3, 5000, nullptr, 22050, true, -23.0, 1.0));
    std::printf("check legal_smallest %d\n", answer(true, 1, 1, nullptr, 8000, true, -70.0, 1e-9));
    std::printf("check legal_largest %d\n", answer(true, 1, 2147483647, nullptr, 192000, true, 0.0, 1e9));
    std::printf("check legal_measure_ignores_target %d\n", answer(true, 1, 10, nullptr, 48000, false, nan, -1.0));
    std::printf("check null %d\n", answer(false, 3, 5000, nullptr, 22050, false, 0.0, 1.0));
    std::printf("check null_normalize %d\n", answer(false, 3, 5000, nullptr, 22050, true, -23.0, 1.0));
    std::printf("check B0 %d\n", answer(true, 0, 5000, nullptr, 22050, false, 0.0, 1.0));
    std::printf("check N0 %d\n", answer(true, 3, 0, nullptr, 22050, false, 0.0, 1.0));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(true, 3, 5000, &l, 22050, false, 0.0, 1.0));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }
    std::printf("check target_nan %d\n", answer(true, 3, 5000, nullptr, 22050, true, nan, 1.0));
    std::printf("check target_inf %d\n", answer(true, 3, 5000, nullptr, 22050, true, -inf, 1.0));
    std::printf("check peak0 %d\n", answer(true, 3, 5000, nullptr, 22050, true, -23.0, 0.0));
    std::printf("check peak_negative %d\n", answer(true, 3, 5000, nullptr, 22050, true, -23.0, -1.0));
    std::printf("check peak_nan %d\n", answer(true, 3, 5000, nullptr, 22050, true, -23.0, nan));
    std::printf("check peak_inf %d\n", answer(true, 3, 5000, nullptr, 22050, true, -23.0, inf));
    std::printf("check sr_below_above %d\n", answer(true, 3, 5000, nullptr, 7999, false, 0.0, 1.0));
    std::printf("check sr_beyond_above %d\n", answer(true, 3, 5000, nullptr, 192001, true, -23.0, 1.0));
    std::printf("check sr0_above %d\n", answer(true, 3, 5000, nullptr, 0, false, 0.0, 1.0));
    std::printf("check sr_negative_above %d\n", answer(true, 3, 5000, nullptr, -22050, false, 0.0, 1.0));
    // tts_set_loudness asks the same checks of (target, max_peak, sampling rate) alone
    std::printf("check legal_setting %d\n", answer(true, 1, 1, nullptr, 22050, true, -16.0, 0.9));
    std::printf("check setting_sr_above %d\n", answer(true, 1, 1, nullptr, 200000, true, -16.0, 0.9));
    return exit_status();
}
