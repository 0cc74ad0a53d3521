// The dynamics compressor, host side: a feed-forward peak compressor over batches of mono waveforms -- the arithmetic every side
// runs (host, kernel and tests/compressor_oracle.py share this one definition), the design of the two coefficients, the named
// profiles, the cut of a row into segments and the argument checks of tts_compress and tts_set_compressor.  Plain C++ (no HIP, no
// handle): compressor.hip includes it, and tests/compressor_check.cpp compiles it alone.
//
// A sample x (a double), the states e1 (release) and e (attack), both 0 in front of a row:
//   v  = |x|, or 0 where x is not finite
//   e1 = max(v, aR e1)                         one product
//   e  = aA e + bA e1                          two products and a sum, each individually rounded; bA = 1 - aA rounded once on the host
//   L  = 20 log10(e),  d = L - T
//   r  = 0                                     where 2 d <= -W
//      = (s - 1) d                             where 2 d >= W
//      = (s - 1) (d + W / 2)^2 / (2 W)         between them (W > 0)
//   out = x's own bits where r + makeup == 0, else float32(x * 10^((r + makeup) / 20)), rounded once
// r is computed directly, so e = 0 (L = -inf) gives r = 0.
// The cut is the equaliser's (equalizer_plan.h): segments of EQ_SEG samples, EQ_TILE_SEGS of them a tile.  Both recurrences compose
// in closed form over a segment -- y -> max(c, AR y) for e1 (an incoming release trajectory that a peak of the segment overtakes
// stays overtaken) and y -> AA y + q for e, AR and AA being aR and aA multiplied out EQ_SEG times (cmp_power) -- so:
//   pass A   every segment but the row's last from e1 = 0: keeps c, the e1 it ends in
//   chain A  s[0] = 0, s[k+1] = max(c[k], AR s[k])
//   pass B   every segment but the row's last from e1 = s[k] and e = 0: keeps q, the e it ends in (q depends on the true e1)
//   chain B  t[0] = 0, t[k+1] = AA t[k] + q[k]      a product and a sum
//   pass C   every segment from e1 = s[k], e = t[k]: the gain, the output
#pragma once
#include "equalizer_plan.h"

namespace tts {

constexpr double CMP_THRESHOLD_MIN = -80.0, CMP_THRESHOLD_MAX = 0.0;   // dB re full scale
constexpr double CMP_KNEE_MAX = 40.0;                                  // dB, the knee's whole width
constexpr double CMP_MAKEUP_MIN = -24.0, CMP_MAKEUP_MAX = 24.0;        // dB
constexpr double CMP_MS_MAX = 10000.0;                                 // the design: attack and release, ms
constexpr int CMP_UTTS = EQ_UTTS;

// (the public tts_compressor_t, field for field; include/sstts_hip.h)
struct CmpParams {
    double threshold_db, slope, knee_db, makeup_db, attack_coeff, release_coeff;
};

// what travels to the kernels by value
struct CmpCoef {
    double T, s1 /* slope - 1 */, W, makeup, aA, bA, aR, AA, AR;
};

// a multiplied out EQ_SEG times, one rounded product a time
constexpr double cmp_power(double a) {
    double p = 1.0;
    for (int i = 0; i < EQ_SEG; ++i) p = p * a;
    return p;
}

inline CmpCoef cmp_coef(const CmpParams& p) {
    return CmpCoef{p.threshold_db, p.slope - 1.0, p.knee_db, p.makeup_db, p.attack_coeff, 1.0 - p.attack_coeff, p.release_coeff,
                   cmp_power(p.attack_coeff), cmp_power(p.release_coeff)};
}

// doubles of workspace for a row of N samples: [2][eq_segments(N)], c -> s and q -> t
constexpr size_t cmp_state_doubles(int N) { return (size_t)eq_segments(N) * 2; }
// the partial records of a row of N samples: one a tile
constexpr size_t cmp_partials(int N) { return (size_t)eq_tiles(N); }

// ---- the arithmetic
// the detector: one sample into both states; returns e
#if defined(__HIPCC__)
__host__ __device__
#endif
inline double cmp_detect(const CmpCoef& k, double x, double& e1, double& e) {
    const double ax = fabs(x);
    const double v = ax <= 1.7976931348623157e308 ? ax : 0.0;   // (a NaN compares false)
    const double rel = k.aR * e1;
    e1 = v > rel ? v : rel;
    const double p = k.aA * e, q = k.bA * e1;
    e = p + q;
    return e;
}

// the gain reduction in dB (<= 0) at the level L = 20 log10(e)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline double cmp_reduction(const CmpCoef& k, double L) {
    const double d = L - k.T, d2 = 2.0 * d;
    if (d2 <= -k.W) return 0.0;
    if (d2 >= k.W) return k.s1 * d;
    const double u = d + k.W / 2.0;
    return k.s1 * (u * u) / (2.0 * k.W);
}

// The plain restatement of the five passes for one row (the check program): out, and env[n] where env is given.
inline void cmp_row(const CmpParams& p, const float* x, long long n, float* out, double* env) {
    const CmpCoef k = cmp_coef(p);
    double s = 0.0, t = 0.0;
    for (long long i = 0; i < eq_segments(n); ++i) {
        const int len = eq_segment_len(n, i);
        double e1 = s, e = t;
        for (int j = 0; j < len; ++j) {
            const float xf = x[i * EQ_SEG + j];
            const double ev = cmp_detect(k, (double)xf, e1, e);
            if (env) env[i * EQ_SEG + j] = ev;
            const double z = cmp_reduction(k, 20.0 * std::log10(ev)) + k.makeup;
            out[i * EQ_SEG + j] = z == 0.0 ? xf : (float)((double)xf * std::pow(10.0, z / 20.0));
        }
        if (i + 1 < eq_segments(n)) {
            double c = 0.0, unused = 0.0, q = 0.0;
            for (int j = 0; j < len; ++j) cmp_detect(k, (double)x[i * EQ_SEG + j], c, unused);
            e1 = s;
            for (int j = 0; j < len; ++j) cmp_detect(k, (double)x[i * EQ_SEG + j], e1, q);
            const double rel = k.AR * s;
            s = c > rel ? c : rel;
            const double pr = k.AA * t;
            t = pr + q;
        }
    }
}

// ---- the design: a time constant in ms at a sampling rate as a one-pole coefficient, exp(-1 / (ms 1e-3 sr)); 0 ms: 0
inline std::string cmp_design(int sr, double attack_ms, double release_ms, double* attack_coeff, double* release_coeff) {
    if (sr < EQ_SR_MIN || sr > EQ_SR_MAX)
        return "the sampling rate " + std::to_string(sr) + " is not in " + std::to_string(EQ_SR_MIN) + " .. " + std::to_string(EQ_SR_MAX);
    std::string bad = eq_range("the attack in ms,", attack_ms, 0.0, CMP_MS_MAX);
    if (bad.empty()) bad = eq_range("the release in ms,", release_ms, 0.0, CMP_MS_MAX);
    if (!bad.empty()) return bad;
    *attack_coeff = attack_ms == 0.0 ? 0.0 : std::exp(-1.0 / (attack_ms * 1e-3 * (double)sr));
    *release_coeff = release_ms == 0.0 ? 0.0 : std::exp(-1.0 / (release_ms * 1e-3 * (double)sr));
    return std::string();
}

// ---- the profiles: a function of a name and the sampling rate.  Every preset is untuned.
struct CmpProfile {
    const char* name;
    double threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db;
};
constexpr int CMP_PROFILES = 3;
inline const CmpProfile* cmp_profiles() {
    static const CmpProfile table[CMP_PROFILES] = {
        {"speech", -18.0, 3.0, 6.0, 5.0, 100.0, 3.0},
        {"telephony", -20.0, 4.0, 6.0, 3.0, 80.0, 6.0},
        {"small-speaker", -24.0, 6.0, 10.0, 2.0, 60.0, 8.0},
    };
    return table;
}

// ---- the argument checks
inline std::string cmp_params_check(const CmpParams& p) {
    std::string bad = eq_range("threshold_db =", p.threshold_db, CMP_THRESHOLD_MIN, CMP_THRESHOLD_MAX);
    if (bad.empty()) bad = eq_range("slope =", p.slope, 0.0, 1.0);
    if (bad.empty()) bad = eq_range("knee_db =", p.knee_db, 0.0, CMP_KNEE_MAX);
    if (bad.empty()) bad = eq_range("makeup_db =", p.makeup_db, CMP_MAKEUP_MIN, CMP_MAKEUP_MAX);
    if (bad.empty() && !(p.attack_coeff >= 0.0 && p.attack_coeff < 1.0)) bad = "attack_coeff is not in [0, 1)";
    if (bad.empty() && !(p.release_coeff >= 0.0 && p.release_coeff < 1.0)) bad = "release_coeff is not in [0, 1)";
    return bad;
}

// Why a profile is refused (*invalid: an unknown name or a NULL pointer, TTS_ERR_INVALID; else TTS_ERR_UNSUPPORTED: the sampling
// rate); empty: *out is written.
inline std::string cmp_profile(const char* name, int sr, CmpParams* out, bool* invalid) {
    *invalid = true;
    if (!name || !out) return "a NULL pointer (name and params_out are required)";
    const CmpProfile* p = nullptr;
    for (int i = 0; i < CMP_PROFILES; ++i)
        if (!std::strcmp(name, cmp_profiles()[i].name)) p = cmp_profiles() + i;
    if (!p) {
        std::string all;
        for (int i = 0; i < CMP_PROFILES; ++i) all += std::string(i ? ", " : "") + cmp_profiles()[i].name;
        return "no profile '" + std::string(name) + "' (there are: " + all + ")";
    }
    *invalid = false;
    CmpParams q{p->threshold_db, 1.0 / p->ratio, p->knee_db, p->makeup_db, 0.0, 0.0};
    const std::string bad = cmp_design(sr, p->attack_ms, p->release_ms, &q.attack_coeff, &q.release_coeff);
    if (!bad.empty()) return "the profile '" + std::string(name) + "': " + bad;
    *out = q;
    return std::string();
}

// The checks of tts_compress in the order the header lists them; wav, out, envelope: the addresses.  Empty: the call is legal.
inline std::string compressor_check(uintptr_t wav, uintptr_t out, int B, int N, const int32_t* n_samples, const CmpParams* p, uintptr_t envelope) {
    if (!wav || !out || !p) return "a NULL pointer (wav, out and params are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N);
    if (bad.empty()) bad = cmp_params_check(*p);
    if (!bad.empty()) return bad;
    // (the envelope's alignment stands between the pair's alignment and its overlap)
    if (!((wav | out) & 3) && (envelope & 7)) return "envelope must be 8-byte aligned";
    return in_out_refusal(wav, out, B, N);
}

}  // namespace tts
