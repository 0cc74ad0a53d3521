// Band-limited resampling, host side: the filter design, the lengths of a resampled utterance, the constants of a ratio and the
// argument checks of tts_resample.  Plain C++ (no HIP, no handle): resample.hip and the pipeline include it, and
// tests/resample_check.cpp compiles it alone.
//   librosa 0.6 resample(..., res_type='kaiser_best') = resampy 0.2 resample_f with the 'kaiser_best' filter, which
//   pitch_shift (reference audio/effects.py:9-43) and load_wav(sampling_rate=...) run.
// resampy ships the filter as a data file; it is regenerated here from the published design parameters.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace tts {

constexpr double RESAMPLE_RATIO_MIN = 0.25, RESAMPLE_RATIO_MAX = 4.0;
constexpr int RS_NUM_ZEROS = 64;
constexpr int RS_NUM_TABLE = 512;                         // 2 ** precision, precision = 9
constexpr int RS_HALF = RS_NUM_TABLE * RS_NUM_ZEROS;      // n: the half window has n + 1 samples
constexpr int RS_NWIN = RS_HALF + 1;                      // 32769
constexpr double RS_BETA = 14.769656459379492;
constexpr double RS_ROLLOFF = 0.9475937167399596;

// a NaN fails both comparisons
inline bool resample_ratio_ok(double rho) { return rho >= RESAMPLE_RATIO_MIN && rho <= RESAMPLE_RATIO_MAX; }

// resampy writes (long long)(n * rho) samples -- a product in double, truncated; 0 for n < 1
inline long long resampled_valid(int n, double rho) {
    if (n < 1) return 0;
    return (long long)((double)n * rho);
}

// ... and librosa (fix=True) zero-pads them to ceil(n * rho)
inline long long resampled_length(int n, double rho) {
    if (n < 1) return 0;
    return (long long)std::ceil((double)n * rho);
}

// The modified Bessel function I0 by its power series, sum ((x / 2) ** 2k / (k!) ** 2): every term is positive, so the sum is
// good to a few ulp for the arguments met here (0 .. beta).
inline double rs_bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// The half window before the ratio's scale: kaiser(2 n + 1, beta)[n + j] * rolloff * sinc(rolloff * j / 512), j = 0 .. n, with
// numpy's kaiser (i0(beta sqrt(1 - (j / n) ** 2)) / i0(beta)) and numpy's sinc (sin(pi x) / (pi x), x = 0 read as 1e-20).
inline std::vector<double> resample_half_window() {
    std::vector<double> win((size_t)RS_NWIN);
    const double i0b = rs_bessel_i0(RS_BETA);
    for (int j = 0; j <= RS_HALF; ++j) {
        const double r = (double)j / (double)RS_HALF;
        const double kaiser = rs_bessel_i0(RS_BETA * std::sqrt(1.0 - r * r)) / i0b;
        const double x = RS_ROLLOFF * (double)j / (double)RS_NUM_TABLE;
        const double y = M_PI * (x == 0.0 ? 1.0e-20 : x);
        win[(size_t)j] = kaiser * RS_ROLLOFF * (std::sin(y) / y);
    }
    return win;
}

// The constants of a ratio rho = target rate / source rate.
struct ResampleConsts {
    double scale = 1.0;   // min(1, rho)
    double inc = 1.0;     // 1 / rho: the input samples between two outputs
    int step = 0;         // (int)(scale * 512): the table samples between two taps.  The truncation is resampy's
    int phases = 0;       // step + 1: off = (int)(frac * 512) lies in [0, step] on both wings
    int taps_max = 0;     // 32769 / step: the taps of a wing at off = 0
    int row = 0;          // taps_max rounded up to 8: the taps a row of the phase-major table has room for (128-byte rows)
};

inline ResampleConsts resample_consts(double rho) {
    ResampleConsts c;
    c.scale = rho < 1.0 ? rho : 1.0;
    c.inc = 1.0 / rho;
    c.step = (int)(c.scale * (double)RS_NUM_TABLE);
    c.phases = c.step + 1;
    c.taps_max = RS_NWIN / c.step;
    c.row = (c.taps_max + 7) / 8 * 8;
    return c;
}

// The taps of a wing whose first table sample is `off`: (32769 - off) / step, before the signal's ends cut it
inline int resample_wing_taps(int off, int step) { return (RS_NWIN - off) / step; }

// Where output sample t sits: m the input sample at or before it, then per wing the first table sample, the interpolation
// weight and the taps.  Every operation is a double operation rounded on its own; resample.hip computes the same.
struct ResamplePhase {
    long long m = 0;
    int off[2] = {0, 0};
    double eta[2] = {0.0, 0.0};
    int taps[2] = {0, 0};   // cut at the ends of an utterance of n_in samples
};

inline ResamplePhase resample_phase(long long t, int n_in, const ResampleConsts& c) {
    ResamplePhase p;
    const double tr = (double)t * c.inc;
    p.m = (long long)tr;
    double frac = c.scale * (tr - (double)p.m);
    for (int wing = 0; wing < 2; ++wing) {
        if (wing == 1) frac = c.scale - frac;
        const double f = frac * (double)RS_NUM_TABLE;
        p.off[wing] = (int)f;
        p.eta[wing] = f - (double)p.off[wing];
        const long long room = wing == 0 ? p.m + 1 : (long long)n_in - p.m - 1;
        const long long taps = resample_wing_taps(p.off[wing], c.step);
        p.taps[wing] = (int)(room < taps ? (room < 0 ? 0 : room) : taps);
    }
    return p;
}

// The half window of a ratio (win *= rho below 1) and its differences, delta[n] = 0
inline void resample_scaled_window(const std::vector<double>& base, double rho, std::vector<double>& win, std::vector<double>& delta) {
    win = base;
    if (rho < 1.0)
        for (double& w : win) w *= rho;
    delta.assign(win.size(), 0.0);
    for (size_t j = 0; j + 1 < win.size(); ++j) delta[j] = win[j + 1] - win[j];
}

// The phase-major copy: tab[(off * row + i) * 2 + {0, 1}] = win / delta at off + i * step, i < (32769 - off) / step, zeros behind.
// A lane's taps are then contiguous.
inline std::vector<double> resample_phase_table(const std::vector<double>& base, double rho, const ResampleConsts& c) {
    std::vector<double> win, delta;
    resample_scaled_window(base, rho, win, delta);
    std::vector<double> tab((size_t)c.phases * c.row * 2, 0.0);
    for (int off = 0; off < c.phases; ++off) {
        const int taps = resample_wing_taps(off, c.step);
        for (int i = 0; i < taps; ++i) {
            const size_t j = (size_t)off + (size_t)i * c.step;
            tab[((size_t)off * c.row + i) * 2] = win[j];
            tab[((size_t)off * c.row + i) * 2 + 1] = delta[j];
        }
    }
    return tab;
}

// The checks of tts_resample, in the order the header lists them; an empty string: the call is legal.  n_samples: host lengths
// or null (all n).  have_ptrs: the data pointers are not NULL.
inline std::string resample_check(bool have_ptrs, int B, int n, const int32_t* n_samples, double rho, int N_out) {
    if (!have_ptrs) return "a NULL pointer";
    if (!resample_ratio_ok(rho)) return "the ratio must be finite and lie in [0.25, 4]";
    if (B < 1 || n < 1 || N_out < 1) return "need B, n, N_out >= 1";
    return lengths_refusal("n_samples", n_samples, B, "n", n);
}

}  // namespace tts
