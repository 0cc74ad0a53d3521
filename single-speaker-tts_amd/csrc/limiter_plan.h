// The look-ahead peak limiter and the true-peak meter, host side: the interpolation taps, the gain rule every side runs (kernel
// and tests/limiter_oracle.py share this one definition), the tile and halo arithmetic of the kernels and the argument checks of
// tts_true_peak, tts_limit and tts_set_limiter.  Plain C++ (no HIP, no handle): limiter.hip includes it, and
// tests/limiter_check.cpp compiles it alone.
//
// The 4x oversampled signal of an utterance x[0 .. n): y[4 i] = x[i], and for p = 1 .. 3
//   y[4 i + p] = sum over k = 0 .. 11, ascending, of h[p][k] * x[i - 5 + k]        (samples outside 0 .. n - 1 are zero)
// the first product alone, then a sum per further product.  h[p][k] = sinc(t) * kaiser(t / 6), t = (k - 5) - p / 4, is a Kaiser
// windowed sinc, LIM_BETA its one shape parameter; phase 0 is the unit impulse exactly.
// The envelope a[i]: |x[i]| (oversample 1), or the largest finite |y[4 i + p]|, p = 0 .. 3 (oversample 4); 0 for a non-finite x[i]
// whatever its neighbours.  A non-finite sample makes the interpolated points within its taps' reach non-finite: those are skipped.
// The limiter, for a ceiling c and a look-ahead of L samples:
//   r[i] = a[i] > c ? c / a[i] : 1                                                  the required gain
//   m[i] = min r[j], |j - i| <= L, j in 0 .. n - 1                                  exact: any algorithm
//   s[i] = (m[cl(i - L)] + m[cl(i - L + 1)] + ... + m[cl(i + L)]) / (2 L + 1)       ascending, cl(j) = min(max(j, 0), n - 1)
//   g[i] = min(s[i], r[i])
//   out[i] = x[i]'s bits where g[i] == 1 or x[i] is not finite, else copysign(min(|(float)(g[i] * (double)x[i])|, cf), x[i]),
//   cf the largest float <= c.
// Every product, sum and quotient is an individually rounded IEEE double operation.
#pragma once
#include "lengths.h"
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int LIM_MAX_LOOKAHEAD = 1024;
constexpr int LIM_PHASES = 4, LIM_TAPS = 12, LIM_BEFORE = 5, LIM_AFTER = 6;   // a point reads x[i - 5 .. i + 6]
constexpr double LIM_BETA = 4.0;
constexpr int LIM_UTTS = 64;      // utterances per launch: their lengths travel by value
constexpr int LIM_TILE = 2048;    // samples a workgroup owns
constexpr int LIM_LANES = 256;
constexpr int LIM_PER_LANE = LIM_TILE / LIM_LANES;   // samples of the tile a lane owns, LIM_LANES apart

struct LimTaps {
    double h[LIM_PHASES * LIM_TAPS];   // [phase][tap]
};

// I0 by its power series (every term is positive: good to a few ulp for 0 .. beta)
inline double lim_bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

inline LimTaps lim_taps() {
    LimTaps t;
    const double pi = 3.141592653589793, i0b = lim_bessel_i0(LIM_BETA);
    for (int p = 0; p < LIM_PHASES; ++p)
        for (int k = 0; k < LIM_TAPS; ++k) {
            double v = k == LIM_BEFORE ? 1.0 : 0.0;
            if (p) {
                const double d = (double)(k - LIM_BEFORE) - 0.25 * (double)p, u = d / (double)LIM_AFTER;
                v = std::sin(pi * d) / (pi * d) * (lim_bessel_i0(LIM_BETA * std::sqrt(1.0 - u * u)) / i0b);
            }
            t.h[p * LIM_TAPS + k] = v;
        }
    return t;
}

// the largest float <= c (c finite and positive)
inline float lim_ceiling_float(double c) {
    if (c >= (double)FLT_MAX) return FLT_MAX;
    float f = (float)c;
    if ((double)f > c) f = std::nextafterf(f, 0.f);
    return f;
}

// The tile of a workgroup: samples [first, first + LIM_TILE) of an utterance.  Its gains read r over 2 L samples either side
// (the minimum's L, then the mean's L) and r reads x over 5 before and 6 after: LDS holds x from lim_x_first on, lim_x_count of
// them, r from lim_r_first on, lim_r_count of them.
constexpr long long lim_tiles(long long n) { return (n + LIM_TILE - 1) / LIM_TILE; }
constexpr int lim_r_count(int L) { return LIM_TILE + 4 * L; }
constexpr int lim_x_count(int L) { return lim_r_count(L) + LIM_BEFORE + LIM_AFTER; }
constexpr long long lim_r_first(long long first, int L) { return first - 2 * (long long)L; }
constexpr long long lim_x_first(long long first, int L) { return lim_r_first(first, L) - LIM_BEFORE; }
// three arrays: x (later a scratch of the minimum), r, and the minimum's other scratch
constexpr size_t lim_lds_bytes(int L) { return ((size_t)lim_x_count(L) + 2 * (size_t)lim_r_count(L)) * sizeof(double); }
constexpr size_t LIM_LDS_MAX = 160 * 1024;
static_assert(lim_lds_bytes(LIM_MAX_LOOKAHEAD) <= LIM_LDS_MAX, "the largest look-ahead fits the LDS of a compute unit");

// The sliding minimum by doubling: after lim_min_steps(W) doublings a cell holds the minimum of lim_min_span(W) cells from it on,
// the largest power of two <= W = 2 L + 1; two of those, W - span apart, cover the window.
constexpr int lim_min_steps(int W) {
    int s = 0;
    while ((2 << s) <= W) ++s;
    return s;
}
constexpr int lim_min_span(int W) { return 1 << lim_min_steps(W); }

// The checks of tts_true_peak (limit = false: ceiling, lookahead and oversample are not looked at), tts_limit and -- with
// have_ptrs = true, B = N = 1 and no lengths -- tts_set_limiter, in the order the header lists them.  An empty string: legal.
inline std::string limiter_check(bool have_ptrs, int B, int N, const int32_t* n_samples, bool limit, double ceiling, int lookahead, int oversample) {
    if (!have_ptrs) return limit ? "a NULL pointer (wav is required)" : "a NULL pointer (wav and true_peak are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    if (limit) {
        if (!(std::isfinite(ceiling) && ceiling > 0.0)) return "the ceiling must be finite and positive";
        if (lookahead < 0 || lookahead > LIM_MAX_LOOKAHEAD) return "the look-ahead " + std::to_string(lookahead) + " is not in 0 .. " + std::to_string(LIM_MAX_LOOKAHEAD);
        if (oversample != 1 && oversample != 4) return "oversample must be 1 or 4";
    }
    return lengths_refusal("n_samples", n_samples, B, "N", N);
}

}  // namespace tts
