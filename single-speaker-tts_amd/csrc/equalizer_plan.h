// The equaliser, host side: a cascade of up to EQ_MAX_SECTIONS second-order sections over batches of mono waveforms -- the design
// of a section (low-pass, high-pass, peak, shelves) and of the named profiles, the recurrence every side runs (host, kernel and
// tests/equalizer_oracle.py share this one definition), the cut of a row into segments and the argument checks of tts_equalize and
// tts_set_equalizer.  Plain C++ (no HIP, no handle): equalizer.hip includes it, and tests/equalizer_check.cpp compiles it alone.
//
// A section is b0 b1 b2 a1 a2, normalised by a0; a sample runs through the cascade in direct form II transposed (eq_sample), the
// state of S sections is the 2 S values z1, z2 of section 0, then of section 1, ...
// The cut: a row of n samples is eq_segments(n) = ceil(n / EQ_SEG) segments of EQ_SEG samples, the last one of 1 .. EQ_SEG; it
// does not depend on the sampling rate.
//   pass 1  runs the cascade over each segment but the row's last from the zero state and keeps the 2 S state values it ends in,
//           e_i (nothing reads the last segment's end state).
//   pass 2  chains them along the row, S_0 = 0 and, for row r of the 2 S x 2 S transition M of EQ_SEG samples (eq_transition),
//             S_{i+1}[r] = ((((M[r][0] S_i[0] + M[r][1] S_i[1]) + M[r][2] S_i[2]) + ... + M[r][2 S - 1] S_i[2 S - 1]) + e_i[r]
//           the first product alone, a sum per further product in ascending column order, e_i[r] last (eq_chain).
//   pass 3  runs each segment again from S_i and rounds each y to float32 once.
// Every product and sum is an individually rounded IEEE double operation.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace tts {

constexpr int EQ_MAX_SECTIONS = 8;
constexpr int EQ_SEG = 256;          // samples of a segment: one lane owns one
constexpr int EQ_TILE_SEGS = 64;     // segments a workgroup stages through LDS
constexpr int EQ_TILE = EQ_TILE_SEGS * EQ_SEG;
constexpr int EQ_LDS_STRIDE = EQ_SEG + 1;   // floats between two segments of a tile in LDS: the 64 lanes of a step hit 64 banks
constexpr int EQ_UTTS = 64;          // utterances per launch: their lengths travel by value
constexpr int EQ_SR_MIN = 8000, EQ_SR_MAX = 192000;
constexpr double EQ_F_MIN = 1e-4, EQ_F_MAX = 0.49;   // f0 / sr
constexpr double EQ_Q_MIN = 0.1, EQ_Q_MAX = 30.0;
constexpr double EQ_GAIN_MIN = -40.0, EQ_GAIN_MAX = 24.0;   // dB
constexpr double EQ_Q_BUTTER2 = 0.7071067811865476;         // one section: a 2nd-order Butterworth; the shelves' default
constexpr double EQ_Q_BUTTER4[2] = {0.5411961001461969, 1.3065629648763766};   // two sections: a 4th-order Butterworth

enum EqKind { EQ_LOWPASS = 0, EQ_HIGHPASS = 1, EQ_PEAK = 2, EQ_LOWSHELF = 3, EQ_HIGHSHELF = 4, EQ_KINDS = 5 };

constexpr size_t eq_lds_bytes() { return (size_t)EQ_TILE_SEGS * EQ_LDS_STRIDE * sizeof(float); }
static_assert(eq_lds_bytes() <= 80 * 1024, "two tiles fit the 160 KB of LDS of a compute unit");

// (constexpr: the kernels call these too)
constexpr long long eq_segments(long long n) { return (n + EQ_SEG - 1) / EQ_SEG; }
constexpr int eq_segment_len(long long n, long long i) { return (int)(n - i * EQ_SEG < EQ_SEG ? n - i * EQ_SEG : EQ_SEG); }
constexpr long long eq_tiles(long long n) { return (n + EQ_TILE - 1) / EQ_TILE; }
// doubles of workspace: the states of a row of N samples, [2 S][eq_segments(N)] (component-major: the lanes of a wave own
// neighbouring segments), and the transition
constexpr size_t eq_state_doubles(int N, int S) { return (size_t)eq_segments(N) * 2 * (size_t)S; }
constexpr size_t eq_transition_doubles(int S) { return (size_t)(2 * S) * (size_t)(2 * S); }

// One sample through a cascade of S sections k[S][5], direct form II transposed; st[S][2].  Returns y.
constexpr double eq_sample(const double* k, int S, double* st, double x) {
    for (int s = 0; s < S; ++s) {
        const double* c = k + 5 * s;
        double* z = st + 2 * s;
        const double y = c[0] * x + z[0];
        z[0] = (c[1] * x - c[3] * y) + z[1];
        z[1] = c[2] * x - c[4] * y;
        x = y;
    }
    return x;
}

// The transition of EQ_SEG samples, row-major M[r][j], 2 S x 2 S: column j is the state the recurrence ends in from the unit
// state j on zero input.
inline void eq_transition(const double* k, int S, double* M) {
    const int D = 2 * S;
    for (int j = 0; j < D; ++j) {
        double st[2 * EQ_MAX_SECTIONS] = {};
        st[j] = 1.0;
        for (int i = 0; i < EQ_SEG; ++i) eq_sample(k, S, st, 0.0);
        for (int r = 0; r < D; ++r) M[D * r + j] = st[r];
    }
}

// One link of the chain of pass 2: st <- M st + e.
inline void eq_chain(const double* M, int S, const double* e, double* st) {
    const int D = 2 * S;
    double n[2 * EQ_MAX_SECTIONS] = {};
    for (int r = 0; r < D; ++r) {
        double a = M[D * r] * st[0];
        for (int j = 1; j < D; ++j) a = a + M[D * r + j] * st[j];
        n[r] = a + e[r];
    }
    for (int r = 0; r < D; ++r) st[r] = n[r];
}

// The plain restatement of the three passes for one row (the check program and the library's host callers of small rows).
inline void eq_filter_row(const double* k, int S, const float* x, long long n, float* out) {
    double M[4 * EQ_MAX_SECTIONS * EQ_MAX_SECTIONS];
    eq_transition(k, S, M);
    double at[2 * EQ_MAX_SECTIONS] = {};
    for (long long i = 0; i < eq_segments(n); ++i) {
        const int len = eq_segment_len(n, i);
        double e[2 * EQ_MAX_SECTIONS] = {}, st[2 * EQ_MAX_SECTIONS];
        for (int r = 0; r < 2 * S; ++r) st[r] = at[r];
        for (int j = 0; j < len; ++j) out[i * EQ_SEG + j] = (float)eq_sample(k, S, st, (double)x[i * EQ_SEG + j]);
        if (i + 1 < eq_segments(n)) {
            for (int j = 0; j < len; ++j) eq_sample(k, S, e, (double)x[i * EQ_SEG + j]);
            eq_chain(M, S, e, at);
        }
    }
}

// ---- the design: the bilinear transform in its tan form, K = tan(pi f0 / sr) (no 1 - cos, which cancels at low f0)
inline std::string eq_range(const char* what, double v, double lo, double hi) {
    if (v >= lo && v <= hi) return std::string();   // (a NaN is outside)
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s %.9g is not in %.9g .. %.9g", what, v, lo, hi);
    return buf;
}

// Why a design is refused (TTS_ERR_UNSUPPORTED; the kind: TTS_ERR_INVALID, *invalid set); empty: sos5 is written.
inline std::string eq_design(int kind, int sr, double f0, double q, double gain_db, double* sos5, bool* invalid) {
    *invalid = false;
    if (kind < 0 || kind >= EQ_KINDS) {
        *invalid = true;
        return "the kind " + std::to_string(kind) + " is not in 0 .. " + std::to_string(EQ_KINDS - 1);
    }
    if (sr < EQ_SR_MIN || sr > EQ_SR_MAX)
        return "the sampling rate " + std::to_string(sr) + " is not in " + std::to_string(EQ_SR_MIN) + " .. " + std::to_string(EQ_SR_MAX);
    // (f0 against the products, so that f0 = EQ_F_MIN * sr and f0 = EQ_F_MAX * sr are inside whatever the quotient rounds to)
    std::string bad;
    if (!(f0 >= EQ_F_MIN * (double)sr && f0 <= EQ_F_MAX * (double)sr)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "f0 / sr = %.9g is not in %.9g .. %.9g", f0 / (double)sr, EQ_F_MIN, EQ_F_MAX);
        bad = buf;
    }
    if (bad.empty()) bad = eq_range("Q =", q, EQ_Q_MIN, EQ_Q_MAX);
    const bool gained = kind >= EQ_PEAK;
    if (bad.empty() && gained) bad = eq_range("the gain in dB,", gain_db, EQ_GAIN_MIN, EQ_GAIN_MAX);
    if (!bad.empty()) return bad;
    const double pi = 3.141592653589793;
    const double K = std::tan(pi * f0 / (double)sr), KK = K * K, KQ = K / q;
    double b0, b1, b2, a0, a1, a2;
    if (kind == EQ_LOWPASS || kind == EQ_HIGHPASS) {
        a0 = 1.0 + KQ + KK;
        a1 = 2.0 * (KK - 1.0);
        a2 = 1.0 - KQ + KK;
        b0 = kind == EQ_LOWPASS ? KK : 1.0;
        b1 = kind == EQ_LOWPASS ? 2.0 * KK : -2.0;
        b2 = b0;
    } else if (kind == EQ_PEAK) {
        const double A = std::pow(10.0, gain_db / 40.0);
        b0 = 1.0 + KQ * A + KK;
        b1 = 2.0 * (KK - 1.0);
        b2 = 1.0 - KQ * A + KK;
        a0 = 1.0 + KQ / A + KK;
        a1 = b1;
        a2 = 1.0 - KQ / A + KK;
    } else {
        const double A = std::pow(10.0, gain_db / 40.0), g = std::sqrt(A) * KQ;
        // p: the side the shelf lifts, u: the other one
        const double p = 1.0 + A * KK, u = A + KK, pm = 2.0 * (A * KK - 1.0), um = 2.0 * (KK - A);
        if (kind == EQ_LOWSHELF) {
            b0 = A * (p + g), b1 = A * pm, b2 = A * (p - g);
            a0 = u + g, a1 = um, a2 = u - g;
        } else {
            b0 = A * (u + g), b1 = A * um, b2 = A * (u - g);
            a0 = p + g, a1 = pm, a2 = p - g;
        }
    }
    sos5[0] = b0 / a0, sos5[1] = b1 / a0, sos5[2] = b2 / a0, sos5[3] = a1 / a0, sos5[4] = a2 / a0;
    return std::string();
}

// ---- the profiles: a function of a name and the sampling rate.  Every preset is untuned.
struct EqProfileSection {
    int kind;
    double f0, q, gain_db;
};
struct EqProfile {
    const char* name;
    int n;
    EqProfileSection s[EQ_MAX_SECTIONS];
};
constexpr int EQ_PROFILES = 5;
inline const EqProfile* eq_profiles() {
    static const EqProfile table[EQ_PROFILES] = {
        {"telephony", 4, {{EQ_HIGHPASS, 300.0, EQ_Q_BUTTER4[0], 0.0}, {EQ_HIGHPASS, 300.0, EQ_Q_BUTTER4[1], 0.0},
                          {EQ_LOWPASS, 3400.0, EQ_Q_BUTTER4[0], 0.0}, {EQ_LOWPASS, 3400.0, EQ_Q_BUTTER4[1], 0.0}}},
        {"small-speaker", 3, {{EQ_HIGHPASS, 150.0, EQ_Q_BUTTER4[0], 0.0}, {EQ_HIGHPASS, 150.0, EQ_Q_BUTTER4[1], 0.0}, {EQ_PEAK, 3000.0, 1.0, 3.0}}},
        {"rumble", 1, {{EQ_HIGHPASS, 20.0, 0.7071, 0.0}}},
        {"bright", 1, {{EQ_HIGHSHELF, 6000.0, EQ_Q_BUTTER2, 3.0}}},
        {"warm", 2, {{EQ_HIGHSHELF, 6000.0, EQ_Q_BUTTER2, -3.0}, {EQ_LOWSHELF, 200.0, EQ_Q_BUTTER2, 2.0}}},
    };
    return table;
}

// Why a profile is refused (*invalid: an unknown name or a NULL pointer, TTS_ERR_INVALID; else TTS_ERR_UNSUPPORTED: the sampling
// rate, or a corner that does not fit under EQ_F_MAX sr -- the message names it); empty: sos [n][5] and *n_sections are written.
inline std::string eq_profile(const char* name, int sr, double* sos, int* n_sections, bool* invalid) {
    *invalid = true;
    if (!name || !sos || !n_sections) return "a NULL pointer (name, sos and n_sections are required)";
    const EqProfile* p = nullptr;
    for (int i = 0; i < EQ_PROFILES; ++i)
        if (!std::strcmp(name, eq_profiles()[i].name)) p = eq_profiles() + i;
    if (!p) {
        std::string all;
        for (int i = 0; i < EQ_PROFILES; ++i) all += std::string(i ? ", " : "") + eq_profiles()[i].name;
        return "no profile '" + std::string(name) + "' (there are: " + all + ")";
    }
    for (int i = 0; i < p->n; ++i) {
        const std::string bad = eq_design(p->s[i].kind, sr, p->s[i].f0, p->s[i].q, p->s[i].gain_db, sos + 5 * i, invalid);
        if (!bad.empty()) return "the profile '" + std::string(name) + "' at " + std::to_string(sr) + " Hz: section " + std::to_string(i) + ": " + bad;
    }
    *n_sections = p->n;
    *invalid = false;
    return std::string();
}

// ---- the argument checks
// Checks 4 .. 6 of tts_equalize, and all of tts_set_equalizer's: the sections alone.
inline std::string eq_sections_check(const double* sos, int n_sections) {
    if (n_sections < 1 || n_sections > EQ_MAX_SECTIONS)
        return "n_sections = " + std::to_string(n_sections) + " is not in 1 .. EQ_MAX_SECTIONS = " + std::to_string(EQ_MAX_SECTIONS);
    for (int i = 0; i < 5 * n_sections; ++i)
        if (!std::isfinite(sos[i])) return "coefficient " + std::to_string(i % 5) + " of section " + std::to_string(i / 5) + " is not finite";
    for (int s = 0; s < n_sections; ++s) {
        const double a1 = sos[5 * s + 3], a2 = sos[5 * s + 4];
        if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
            return "section " + std::to_string(s) + " is not stable: |a2| < 1 and |a1| < 1 + a2 are needed";
    }
    return std::string();
}

// The checks of tts_equalize in the order the header lists them; wav, out: the addresses.  An empty string: the call is legal.
inline std::string equalizer_check(uintptr_t wav, uintptr_t out, int B, int N, const int32_t* n_samples, const double* sos, int n_sections) {
    if (!wav || !out || !sos) return "a NULL pointer (wav, out and sos are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N);
    if (bad.empty()) bad = eq_sections_check(sos, n_sections);
    if (!bad.empty()) return bad;
    return in_out_refusal(wav, out, B, N);
}

}  // namespace tts
