// Stand-alone check of the host side of the resampler (csrc/resample_plan.h compiled as plain C++, no GPU, no library): prints
// the lengths over a grid of (n, rho), samples of the half window and of the per-ratio tables, and (m, off, eta, taps) of chosen
// outputs for tests/test_resample_program.py to hold against the numpy oracle, and runs the argument checks of tts_resample
// through every refusal the header lists.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "resample_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static bool refused(bool ptrs, int B, int n, const int32_t* ns, double rho, int N_out) { return !resample_check(ptrs, B, n, ns, rho, N_out).empty(); }

int main() {
    const double ratios[] = {0.25, 0.5, 0.7937005259840998, 16000.0 / 22050.0, 1.0, 1.189207115002721, 2.0, 4.0};
    const int lengths[] = {1, 2, 3, 63, 64, 100, 441, 700, 5000, 22050, 275000};
    for (double r : ratios)
        for (int n : lengths) std::printf("len %d %.17g %lld %lld\n", n, r, resampled_valid(n, r), resampled_length(n, r));
    expect(resampled_valid(0, 2.0) == 0 && resampled_length(-1, 2.0) == 0, "no samples below one");

    const std::vector<double> base = resample_half_window();
    expect((int)base.size() == RS_NWIN, "32769 window samples");
    for (int j = 0; j < RS_NWIN; j += 97) std::printf("win %d %.17g\n", j, base[(size_t)j]);
    std::printf("win %d %.17g\n", RS_NWIN - 1, base[(size_t)RS_NWIN - 1]);

    for (double r : ratios) {
        const ResampleConsts c = resample_consts(r);
        std::printf("consts %.17g %.17g %.17g %d %d %d\n", r, c.scale, c.inc, c.step, c.taps_max, c.row);
        expect(c.row % 8 == 0 && c.row >= c.taps_max && c.phases == c.step + 1, "rows of whole cache lines");
        const std::vector<double> tab = resample_phase_table(base, r, c);
        expect(tab.size() == (size_t)c.phases * c.row * 2, "table size");
        // every phase's row: a few taps, the last one, and the zeros behind it
        for (int off = 0; off < c.phases; off += (off < 3 ? 1 : 61)) {
            const int taps = resample_wing_taps(off, c.step);
            for (int i : {0, 1, taps / 2, taps - 1})
                std::printf("tab %.17g %d %d %.17g %.17g\n", r, off, i, tab[((size_t)off * c.row + i) * 2], tab[((size_t)off * c.row + i) * 2 + 1]);
            for (int i = taps; i < c.row; ++i)
                expect(tab[((size_t)off * c.row + i) * 2] == 0.0 && tab[((size_t)off * c.row + i) * 2 + 1] == 0.0, "zeros behind a row's taps");
        }
        {
            const int off = c.step, taps = resample_wing_taps(off, c.step);
            std::printf("tab %.17g %d %d %.17g %.17g\n", r, off, taps - 1, tab[((size_t)off * c.row + taps - 1) * 2], tab[((size_t)off * c.row + taps - 1) * 2 + 1]);
        }
        const int n_in = 5000;
        const long long keep = resampled_valid(n_in, r);
        for (long long t : {0LL, 1LL, 2LL, 3LL, 17LL, 255LL, 256LL, 1001LL, keep / 2, keep - 2, keep - 1}) {
            const ResamplePhase p = resample_phase(t, n_in, c);
            std::printf("phase %.17g %d %lld %lld %d %.17g %d %d %.17g %d\n", r, n_in, t, p.m, p.off[0], p.eta[0], p.taps[0], p.off[1], p.eta[1], p.taps[1]);
            expect(p.off[0] >= 0 && p.off[0] <= c.step && p.off[1] >= 0 && p.off[1] <= c.step, "off in [0, step]");
            expect(p.m >= 0 && p.m < n_in, "m inside the utterance");
        }
    }

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    expect(!resample_ratio_ok(nan) && !resample_ratio_ok(inf) && !resample_ratio_ok(-inf), "non-finite ratios");
    expect(!resample_ratio_ok(0.0) && !resample_ratio_ok(0.2) && !resample_ratio_ok(4.5) && !resample_ratio_ok(-1.0), "ratios outside [0.25, 4]");
    expect(resample_ratio_ok(0.25) && resample_ratio_ok(1.0) && resample_ratio_ok(4.0), "the ends of the range are legal");

    const int B = 3, n = 100;
    const std::vector<int32_t> lens = {100, 7, 1};
    expect(!refused(true, B, n, lens.data(), 1.3, 130), "a legal ragged call");
    expect(!refused(true, B, n, nullptr, 0.5, 1), "a legal uniform call, N_out below the resampled length");
    expect(!refused(true, B, n, nullptr, 1.0, 1000), "ratio 1.0 is legal, N_out above the resampled length");
    expect(refused(false, B, n, nullptr, 1.3, 130), "NULL pointer");
    for (double r : {nan, inf, 0.0, 0.2, 4.5}) expect(refused(true, B, n, nullptr, r, 130), "bad ratio");
    expect(refused(true, 0, n, nullptr, 1.3, 130) && refused(true, B, 0, nullptr, 1.3, 130) && refused(true, B, n, nullptr, 1.3, 0), "B, n, N_out below 1");
    for (int bad : {0, -1, n + 1}) {
        std::vector<int32_t> l = lens;
        l[1] = bad;
        expect(refused(true, B, n, l.data(), 1.3, 130), "n_samples outside [1, n]");
        std::printf("msg n_samples=%d %s\n", bad, resample_check(true, B, n, l.data(), 1.3, 130).c_str());
    }
    // the order of the header's list: the pointer before the ratio before the sizes before the lengths
    expect(resample_check(false, 0, 0, nullptr, nan, 0) == "a NULL pointer", "NULL first");
    expect(resample_check(true, 0, 0, nullptr, nan, 0).find("ratio") != std::string::npos, "then the ratio");
    expect(resample_check(true, 0, 0, nullptr, 1.0, 0).find("B, n, N_out") != std::string::npos, "then the sizes");
    return exit_status();
}
