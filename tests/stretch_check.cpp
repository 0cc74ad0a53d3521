// Stand-alone check of the host side of the speaking-rate feature (csrc/stretch_plan.h compiled as plain C++, no GPU, no library):
// prints stretched_frames over a grid of lengths and rates for tests/test_stretch_program.py to hold against numpy, and runs the
// argument checks of the stretch entry points through every refusal the header lists.  Built with -fsanitize=address,undefined
// where the compiler has the runtimes.
#include "stretch_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static bool refused(bool ptrs, int B, int F, int T, int stride, const int32_t* n, double rate, int T_out) {
    return !stretch_check(ptrs, B, F, T, stride, n, rate, T_out).empty();
}

int main() {
    const double rates[] = {0.25, 0.5, 0.75, 0.8, 1.0, 1.25, 1.3, 2.0, 3.7, 4.0};
    for (double r : rates)
        for (int n = 1; n <= 64; ++n) std::printf("%d %.17g %lld\n", n, r, stretched_frames(n, r));
    expect(stretched_frames(0, 1.0) == 0 && stretched_frames(-3, 2.0) == 0, "no frames below one");

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    expect(!stretch_rate_ok(nan) && !stretch_rate_ok(inf) && !stretch_rate_ok(-inf), "non-finite rates");
    expect(!stretch_rate_ok(0.0) && !stretch_rate_ok(0.2) && !stretch_rate_ok(4.5) && !stretch_rate_ok(-1.0), "rates outside [0.25, 4]");
    expect(stretch_rate_ok(0.25) && stretch_rate_ok(1.0) && stretch_rate_ok(4.0), "the ends of the range are legal");

    const int B = 3, F = 5, T = 12;
    const std::vector<int32_t> lens = {12, 7, 1};
    expect(!refused(true, B, F, T, F, lens.data(), 1.3, 10), "a legal ragged call (ceil(12 / 1.3) = 10)");
    expect(!refused(true, B, F, T, F + 3, nullptr, 0.5, 24), "a legal uniform call");
    expect(!refused(true, B, F, T, F, nullptr, 1.0, T), "rate 1.0 is a legal direct call");
    expect(refused(false, B, F, T, F, nullptr, 1.3, 10), "NULL pointer");
    for (double r : {nan, inf, 0.0, 0.2, 4.5}) expect(refused(true, B, F, T, F, nullptr, r, 1000), "bad rate");
    expect(refused(true, 0, F, T, F, nullptr, 1.3, 10) && refused(true, B, 0, T, 0, nullptr, 1.3, 10) && refused(true, B, F, 0, F, nullptr, 1.3, 10),
           "B, F, T below 1");
    expect(refused(true, B, F, T, F - 1, nullptr, 1.3, 10), "row_stride < F");
    for (int bad : {0, -1, T + 1}) {
        std::vector<int32_t> l = lens;
        l[1] = bad;
        expect(refused(true, B, F, T, F, l.data(), 1.3, 10), "n_frames outside [1, T]");
        std::printf("msg n_frames=%d %s\n", bad, stretch_check(true, B, F, T, F, l.data(), 1.3, 10).c_str());
    }
    expect(refused(true, B, F, T, F, lens.data(), 1.3, 9), "T_out below the longest stretched length");
    expect(refused(true, B, F, T, F, nullptr, 0.5, 23), "T_out below the longest stretched length (slower)");
    {   // only the lengths decide: a short batch fits a short T_out
        const std::vector<int32_t> l = {2, 1, 1};
        expect(!refused(true, B, F, T, F, l.data(), 2.0, 1), "T_out follows the lengths, not T");
    }
    return exit_status();
}
