// Stand-alone check of the host side of F0 tracking (csrc/f0_plan.h compiled as plain C++, no GPU, no library): prints the frame
// counts, the first sample of a frame, the frames a workgroup owns with its LDS bytes, the lag slots and lag bounds, and what tts_f0
// and tts_f0_compare answer to a list of argument sets, for tests/test_f0_program.py to hold against tests/f0_oracle.py.  Built
// with -fsanitize=address,undefined where the compiler has the runtimes.
#include "f0_plan.h"
#include "check_expect.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last f0_answer

// 0: legal, 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
static int f0_answer(bool ptrs, int B, int N, const std::vector<int32_t>* n, double sr, int hop, int W, int lo, int hi, double thr) {
    bool unsupported = false;
    const std::string why = f0_check(ptrs, B, N, n ? n->data() : nullptr, sr, hop, W, lo, hi, thr, &unsupported);
    g_why = why;
    expect(why.empty() ? !unsupported : true, "unsupported is set with a reason only");
    return why.empty() ? 0 : unsupported ? 2 : 1;
}

int main() {
    std::printf("consts %d %d %d %d %d %d %zu\n", F0_MAX_WINDOW, F0_MAX_LAG, F0_LANES, F0_SLOTS, F0_MAX_GROUP, F0_UTTS, F0_LDS_BUDGET);
    expect(F0_LANES * F0_SLOTS == F0_MAX_LAG, "the lanes' slots cover the longest lag");
    expect(F0_LANES % 64 == 0, "whole waves");
    expect(f0_lds_bytes(F0_MAX_WINDOW, F0_MAX_LAG, 1, 1) <= F0_LDS_BUDGET, "one frame at the limits fits the budget");

    for (int hop : {1, 7, 64, 275, 300, 512})
        for (int n : {1, hop - 1, hop, hop + 1, 10 * hop - 1, 10 * hop, 275000})
            if (n >= 1) std::printf("frames %d %d %d\n", n, hop, f0_frames(n, hop));
    for (int t : {0, 1, 5, 1000})
        for (int hop : {1, 275})
            for (int W : {1, 64, 1024})
                for (int hi : {2, 65, 368}) std::printf("first %d %d %d %d %lld\n", t, hop, W, hi, f0_first_sample(t, hop, W, hi));
    expect(f0_first_sample(7810000, 275, 1024, 368) == 7810000LL * 275 - 696, "frame positions beyond 2^31 samples");

    for (int W : {1, 63, 64, 65, 1024, 2048})
        for (int hi : {2, 63, 64, 65, 255, 256, 257, 368, 1024})
            for (int hop : {1, 7, 64, 275, 300, 512, 100000, 2147483647}) {
                const int frames = f0_group_frames(W, hi, hop);
                std::printf("group %d %d %d %d %zu %zu %d %d\n", W, hi, hop, frames, f0_span(W, hi, hop, frames), f0_lds_bytes(W, hi, hop, frames),
                            f0_row_stride(hi), f0_slots(hi));
                expect(frames >= 1 && frames <= F0_MAX_GROUP, "frames per workgroup");
                expect(f0_lds_bytes(W, hi, hop, frames) <= F0_LDS_BUDGET, "the LDS of a workgroup fits the budget");
                expect(frames == F0_MAX_GROUP || f0_lds_bytes(W, hi, hop, frames + 1) > F0_LDS_BUDGET, "no frame more would fit");
                expect(f0_row_stride(hi) % 2 == 1 && f0_row_stride(hi) > hi, "a table row holds the lags 0 .. tau_max on an odd stride");
                expect(f0_slots(hi) >= 1 && f0_slots(hi) <= F0_SLOTS && f0_slots(hi) * F0_LANES >= hi, "every lag has a lane and a slot");
                // the last read of the last frame of a group lies inside the staged span
                expect((size_t)(frames - 1) * hop + (W - 1) + hi < f0_span(W, hi, hop, frames), "reads stay inside the span");
            }
    for (int T : {1, 2, 7, 8, 9, 1001})
        for (int frames : {1, 3, 8}) std::printf("groups %d %d %d\n", T, frames, f0_groups(T, frames));

    for (double sr : {8000.0, 16000.0, 22050.0, 44100.0, 48000.0})
        for (double f : {20.0, 50.0, 60.0, 400.0, 500.0, 30000.0}) std::printf("lags %.17g %.17g %d %d\n", sr, f, f0_tau_min(sr, f), f0_tau_max(sr, f));

    // ---- tts_f0's answers
    const std::vector<int32_t> ls = {5000, 1, 275};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::printf("f0_check legal_ragged %d\n", f0_answer(true, 3, 5000, &ls, 22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check legal_uniform %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check legal_smallest %d\n", f0_answer(true, 1, 1, nullptr, 1.0, 1, 1, 2, 2, 0.0));
    std::printf("f0_check legal_limits %d\n", f0_answer(true, 1, 1, nullptr, 48000.0, 512, F0_MAX_WINDOW, 2, F0_MAX_LAG, inf));
    std::printf("f0_check legal_threshold_minus_inf %d\n", f0_answer(true, 1, 10, nullptr, 48000.0, 5, 10, 2, 9, -inf));
    std::printf("f0_check null %d\n", f0_answer(false, 3, 5000, nullptr, 22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check B0 %d\n", f0_answer(true, 0, 5000, nullptr, 22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check N0 %d\n", f0_answer(true, 3, 0, nullptr, 22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check hop0 %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 0, 1024, 44, 368, 0.1));
    std::printf("f0_check frames_overflow %d\n", f0_answer(true, 1, 2147483647, nullptr, 22050.0, 1, 1024, 44, 368, 0.1));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("f0_check n=%d %d\n", bad, f0_answer(true, 3, 5000, &l, 22050.0, 275, 1024, 44, 368, 0.1));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }
    std::printf("f0_check sr0 %d\n", f0_answer(true, 3, 5000, nullptr, 0.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check sr_negative %d\n", f0_answer(true, 3, 5000, nullptr, -22050.0, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check sr_nan %d\n", f0_answer(true, 3, 5000, nullptr, nan, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check sr_inf %d\n", f0_answer(true, 3, 5000, nullptr, inf, 275, 1024, 44, 368, 0.1));
    std::printf("f0_check threshold_nan %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 1024, 44, 368, nan));
    std::printf("f0_check W_above %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, F0_MAX_WINDOW + 1, 44, 368, 0.1));
    std::printf("f0_check W0_above %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 0, 44, 368, 0.1));
    std::printf("f0_check tau_max_above %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 1024, 44, F0_MAX_LAG + 1, 0.1));
    std::printf("f0_check tau_min1_above %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 1024, 1, 368, 0.1));
    std::printf("f0_check tau_order_above %d\n", f0_answer(true, 3, 5000, nullptr, 22050.0, 275, 1024, 369, 368, 0.1));

    // ---- tts_f0_compare's answers
    expect(f0_compare_check(true, 40, 55, 94, 3).empty() && f0_compare_check(true, 1, 1, 1, 1).empty(), "legal comparisons");
    expect(!f0_compare_check(false, 40, 55, 94, 3).empty(), "NULL pointer");
    expect(!f0_compare_check(true, 0, 55, 94, 3).empty() && !f0_compare_check(true, 40, 0, 94, 3).empty(), "Ta, Tb below 1");
    expect(!f0_compare_check(true, 40, 55, 0, 3).empty() && !f0_compare_check(true, 40, 55, 94, 0).empty(), "rows, B below 1");

    return exit_status();
}
