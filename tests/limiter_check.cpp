// Stand-alone check of the host side of the limiter stage (csrc/limiter_plan.h compiled as plain C++, no GPU, no library): prints
// the taps, the ceiling's float, and per look-ahead the tile's LDS arithmetic -- for tests/test_limiter_program.py to hold against
// tests/limiter_oracle.py -- walks every index the gain kernel forms in its LDS arrays, runs the sliding minimum by doubling in
// the kernel's order against the plain one, and prints what tts_true_peak, tts_limit and tts_set_limiter answer to a list of
// argument sets.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "limiter_plan.h"
#include "check_expect.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// 0: legal, 1: TTS_ERR_INVALID
static int answer(bool ptrs, int B, int N, const std::vector<int32_t>* n, bool limit, double c, int L, int os) {
    g_why = limiter_check(ptrs, B, N, n ? n->data() : nullptr, limit, c, L, os);
    return g_why.empty() ? 0 : 1;
}

// The minimum over [k, k + W) of r, as the kernel takes it: doublings between two arrays (a cell past the end reads 1), then two
// spans W - span apart.  `mc` cells are wanted; every read is checked against the array it goes to.
static std::vector<double> doubled_minimum(const std::vector<double>& r, int W, int mc) {
    const int rc = (int)r.size(), steps = lim_min_steps(W), span = lim_min_span(W);
    expect(span <= W && 2 * span > W, "span is the largest power of two <= W");
    std::vector<double> cur = r, dst(r.size());
    for (int t = 0; t < steps; ++t) {
        const int off = 1 << t;
        for (int k = 0; k < rc; ++k) dst[(size_t)k] = std::min(cur[(size_t)k], k + off < rc ? cur[(size_t)(k + off)] : 1.0);
        cur.swap(dst);
    }
    std::vector<double> m((size_t)mc);
    for (int k = 0; k < mc; ++k) {
        expect(k + W - span + span - 1 < rc, "the second span ends inside r");
        m[(size_t)k] = std::min(cur.at((size_t)k), cur.at((size_t)(k + W - span)));
    }
    return m;
}

int main() {
    std::printf("consts %d %d %d %d %d %.17g %d %d %d\n", LIM_MAX_LOOKAHEAD, LIM_PHASES, LIM_TAPS, LIM_BEFORE, LIM_AFTER, LIM_BETA, LIM_UTTS, LIM_TILE,
                LIM_LANES);
    expect(LIM_BEFORE + 1 + LIM_AFTER == LIM_TAPS, "a point reads 5 before, itself and 6 after");
    expect(LIM_TILE % LIM_LANES == 0, "a lane owns whole strides of the tile");

    const LimTaps t = lim_taps();
    for (int p = 0; p < LIM_PHASES; ++p) {
        std::printf("taps %d", p);
        for (int k = 0; k < LIM_TAPS; ++k) std::printf(" %.17g", t.h[p * LIM_TAPS + k]);
        std::printf("\n");
    }
    // phase 2 is symmetric about its middle, phase 3 is phase 1 reversed
    for (int k = 0; k < LIM_TAPS; ++k) {
        expect(std::fabs(t.h[2 * LIM_TAPS + k] - t.h[2 * LIM_TAPS + LIM_TAPS - 1 - k]) < 1e-15, "phase 2 is symmetric");
        expect(std::fabs(t.h[1 * LIM_TAPS + k] - t.h[3 * LIM_TAPS + LIM_TAPS - 1 - k]) < 1e-15, "phase 3 mirrors phase 1");
    }

    for (double c : {0.5, 0.1, 1.0, 0.8912509381337456, 1e-50, 1e39, 3.4028234663852886e+38, 16777217.0}) {
        const float cf = lim_ceiling_float(c);
        std::printf("ceiling %.17g %.9g\n", c, (double)cf);
        expect((double)cf <= c, "cf is not above c");
        expect(cf == FLT_MAX || (double)std::nextafterf(cf, std::numeric_limits<float>::infinity()) > c, "cf is the largest such float");
    }

    for (int L : {0, 1, 2, 3, 7, 110, 511, 512, 1023, 1024}) {
        const int W = 2 * L + 1, xc = lim_x_count(L), rc = lim_r_count(L), mc = LIM_TILE + 2 * L;
        std::printf("tile %d %d %d %zu %d %d\n", L, xc, rc, lim_lds_bytes(L), lim_min_steps(W), lim_min_span(W));
        expect(lim_lds_bytes(L) <= LIM_LDS_MAX, "the arrays fit the LDS");
        for (long long first : {0LL, (long long)LIM_TILE, 1048576LL * LIM_TILE}) {
            // r[k] is sample lim_r_first + k and reads x over [k, k + 12) of the x array, whose cell k is sample lim_x_first + k
            expect(lim_r_first(first, L) - LIM_BEFORE == lim_x_first(first, L), "x starts 5 before r");
            expect(rc - 1 + LIM_TAPS - 1 < xc, "the last r reads inside x");
            // sample i = first + k of the tile: r at k + 2 L, the mean's window m[i - L .. i + L] at M[k .. k + 2 L]
            expect(LIM_TILE - 1 + 2 * L < rc && LIM_TILE - 1 + 2 * L < mc, "the tile's own r and the last window lie inside");
            expect(mc - 1 + W - 1 < rc, "the last minimum reads inside r");
        }
        // the doubling against the plain minimum, on r with a few dips
        std::vector<double> r((size_t)rc, 1.0);
        for (int k = 0; k < rc; k += 37 + L / 3) r[(size_t)k] = 0.25 + 0.5 * (double)((k * 7919) % 101) / 101.0;
        r[(size_t)rc - 1] = 0.125;
        const std::vector<double> m = doubled_minimum(r, W, mc);
        bool same = true;
        for (int k = 0; k < mc; ++k) same = same && m[(size_t)k] == *std::min_element(r.begin() + k, r.begin() + k + W);
        expect(same, "the doubled minimum is the minimum");
    }
    for (long long n : {1LL, 2047LL, 2048LL, 2049LL, 2147483647LL}) std::printf("tiles %lld %lld\n", n, lim_tiles(n));

    const std::vector<int32_t> ls = {5000, 1, 275};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::printf("check legal_ragged %d\n", answer(true, 3, 5000, &ls, true, 0.5, 110, 4));
    std::printf("check legal_uniform %d\n", answer(true, 3, 5000, nullptr, true, 0.5, 0, 1));
    std::printf("check legal_largest %d\n", answer(true, 1, 2147483647, nullptr, true, 1e30, LIM_MAX_LOOKAHEAD, 4));
    std::printf("check legal_meter_ignores_the_rest %d\n", answer(true, 1, 10, nullptr, false, nan, -1, 3));
    std::printf("check legal_setting %d\n", answer(true, 1, 1, nullptr, true, 0.9, 110, 4));
    std::printf("check null %d\n", answer(false, 3, 5000, nullptr, true, 0.5, 110, 4));
    std::printf("check null_meter %d\n", answer(false, 3, 5000, nullptr, false, 0.5, 110, 4));
    std::printf("check B0 %d\n", answer(true, 0, 5000, nullptr, true, 0.5, 110, 4));
    std::printf("check N0 %d\n", answer(true, 3, 0, nullptr, false, 0.5, 110, 4));
    std::printf("check ceiling0 %d\n", answer(true, 3, 5000, nullptr, true, 0.0, 110, 4));
    std::printf("check ceiling_negative %d\n", answer(true, 3, 5000, nullptr, true, -0.5, 110, 4));
    std::printf("check ceiling_nan %d\n", answer(true, 3, 5000, nullptr, true, nan, 110, 4));
    std::printf("check ceiling_inf %d\n", answer(true, 3, 5000, nullptr, true, inf, 110, 4));
    std::printf("check lookahead_negative %d\n", answer(true, 3, 5000, nullptr, true, 0.5, -1, 4));
    std::printf("check lookahead_beyond %d\n", answer(true, 3, 5000, nullptr, true, 0.5, LIM_MAX_LOOKAHEAD + 1, 4));
    for (int os : {0, 2, 3, 8, -1}) std::printf("check oversample=%d %d\n", os, answer(true, 3, 5000, nullptr, true, 0.5, 110, os));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(true, 3, 5000, &l, true, 0.5, 110, 4));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
        std::printf("check meter_n=%d %d\n", bad, answer(true, 3, 5000, &l, false, 0.5, 110, 4));
    }
    return exit_status();
}
