// The audio watermark, host side: a keyed spread-spectrum carrier under a block envelope, embedded into and searched for in batches
// of mono waveforms -- the constants, the arithmetic every side runs (host, kernel and tests/watermark_oracle.py share this one
// definition), the workspace sizes and the argument checks of tts_watermark_embed, tts_watermark_detect and tts_set_watermark.
// Plain C++ (no HIP, no handle): watermark.hip includes it, and tests/watermark_check.cpp compiles it alone.
//
// The carrier at position p >= 0 (L = chip, C = chips_per_symbol, P = payload_bits):
//   q = p / L, u = q / C, j = u mod P
//   c(q) = +1 / -1 by bit 63 of splitmix64's finaliser of key + 0x9E3779B97F4A7C15 (q + 1)        (0: +1, 1: -1)
//   m(t) = +1 for t < L / 2, else -1, t = p mod L
//   s(p) = c(q) m(p mod L) (1 - 2 bit_j(payload))
// The block envelope of a row of n samples, blocks of WM_BLOCK = 64 samples from its first:
//   E[k] = the largest |x| of the finite samples of block k; 0 where there is none or the block lies outside the row
//   e[i] = min(E[k - 1], E[k], E[k + 1]), k = i / 64                                                float32 values, exact
// Embed:  y[i] = float32(double(x[i]) + (G double(e[i])) s(i)): a product, a product by +-1, a sum, one rounding to float32;
//         x's own bits where x is not finite or G e == 0.
// Detect: v[i] = clamp(rint(64 double(r[i]) / double(e_r[i])), -127, 127), ties to even; 0 where r is not finite, e_r == 0
//         A_f[i] = sum of v[n] m((n + f) mod L) over the samples with (n + f) / L == i, f = d mod L the phase      |A| <= 127 L
//         a_q(d) = A_f[q - d / L], so with the shift w = d / L:
//         S[d][j] = sum over i of c(i + w) A_f[i] for the chips with ((i + w) / C) mod P == j
//         E[d]    = sum over i of A_f[i]^2                      (a function of the phase alone)
//         T[d]    = sum over j of |S[d][j]|
//         offset = the lowest d with the largest T; payload bit j set where S[offset][j] < 0
// Every sum of the detector is an integer sum: exact in int64, whatever the order.
#pragma once
#include "lengths.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define WM_HD __host__ __device__ inline
#else
#define WM_HD inline
#endif

namespace tts {

constexpr int WM_BLOCK = 64;                  // samples of an envelope block
constexpr int WM_BITS_MAX = 32;               // P
constexpr int WM_CHIP_MIN = 2, WM_CHIP_MAX = 16;   // L, even
constexpr int WM_SYMBOL_MAX = 65536;          // C
constexpr double WM_STRENGTH_MAX = 0.25;      // G
constexpr int WM_MAX_OFFSETS = 4096;          // D
constexpr int WM_UTTS = 64;                   // rows of a launch: their lengths travel by value
constexpr int WM_TILE = 4096;                 // samples of a workgroup of the streaming passes (64 blocks)
constexpr int WM_THREADS = 256;               // ... and its threads
constexpr int WM_CORR_THREADS = 128;          // the correlation: threads of a workgroup = shifts x sub-ranges of a tile
constexpr int WM_CORR_TILE = 2048;            // ... and the chips of a tile (int16 in LDS)
constexpr int WM_V_SCALE = 64, WM_V_MAX = 127;

// (the public tts_watermark_t, field for field; include/sstts_hip.h)
struct WmParams {
    uint64_t key;
    uint32_t payload;
    int32_t payload_bits, chip, chips_per_symbol;
    double strength;
};

// ---- the arithmetic
// splitmix64's finaliser of key + golden (q + 1): the form enc_dither uses (encode_plan.h)
WM_HD uint64_t wm_hash(uint64_t key, uint64_t q) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull * (q + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// 1 where c(q) = -1
WM_HD int wm_chip_negative(uint64_t key, uint64_t q) { return (int)(wm_hash(key, q) >> 63); }
// s(p)
WM_HD int wm_carrier(const WmParams& w, uint64_t p) {
    const uint64_t q = p / (uint64_t)w.chip;
    const int j = (int)((q / (uint64_t)w.chips_per_symbol) % (uint64_t)w.payload_bits);
    const int neg = wm_chip_negative(w.key, q) ^ (int)((p % (uint64_t)w.chip) >= (uint64_t)(w.chip / 2)) ^ (int)((w.payload >> j) & 1u);
    return neg ? -1 : 1;
}
// ... the same for a position below 2^32 in 32-bit arithmetic (the embedder: a row holds fewer than 2^31 samples)
WM_HD int wm_carrier_u32(const WmParams& w, uint32_t p) {
    const uint32_t q = p / (uint32_t)w.chip, t = p - q * (uint32_t)w.chip;
    const uint32_t j = (q / (uint32_t)w.chips_per_symbol) % (uint32_t)w.payload_bits;
    const int neg = wm_chip_negative(w.key, q) ^ (int)(t >= (uint32_t)(w.chip / 2)) ^ (int)((w.payload >> j) & 1u);
    return neg ? -1 : 1;
}
// what a sample adds to its block's E: |x|, 0 where x is not finite
WM_HD float wm_magnitude(float x) {
    const float a = fabsf(x);
    return a <= 3.4028234663852886e38f ? a : 0.0f;   // (a NaN compares false)
}
WM_HD float wm_min3(float a, float b, float c) {
    const float m = a < b ? a : b;
    return m < c ? m : c;
}
// the marked sample; *marked: whether it differs from x by rule (a finite x under a non-zero G e)
WM_HD float wm_mark(float x, float e, double G, int s, bool* marked) {
    const double g = G * (double)e;
    *marked = g != 0.0 && wm_magnitude(x) == fabsf(x);
    if (!*marked) return x;
    const double t = g * (double)s;
    return (float)((double)x + t);
}
// v of a received sample under its envelope
WM_HD int wm_v(float r, float e) {
    if (!(e > 0.0f) || wm_magnitude(r) != fabsf(r)) return 0;
    const double z = rint((double)WM_V_SCALE * (double)r / (double)e);
    return z > (double)WM_V_MAX ? WM_V_MAX : z < -(double)WM_V_MAX ? -WM_V_MAX : (int)z;
}

// ---- sizes
constexpr long long wm_blocks(long long n) { return (n + WM_BLOCK - 1) / WM_BLOCK; }
constexpr long long wm_tiles(long long n) { return (n + WM_TILE - 1) / WM_TILE; }
// chip sums of a phase of a row of N samples: positions 0 .. N - 1 + (L - 1), padded to a whole correlation tile
constexpr long long wm_chips(long long N, int L) { return (N + 2 * (long long)L - 2) / L; }
constexpr long long wm_corr_tiles(long long N, int L) { return (wm_chips(N, L) + WM_CORR_TILE - 1) / WM_CORR_TILE; }
constexpr long long wm_chips_padded(long long N, int L) { return wm_corr_tiles(N, L) * WM_CORR_TILE; }
// shifts of whole chips that D offsets reach: d / L for d < D
constexpr int wm_shifts(int D, int L) { return (D - 1) / L + 1; }
// a correlation workgroup: SW shifts (a power of two up to 128) x 128 / SW sub-ranges of a tile
constexpr int wm_corr_shifts(int D, int L) {
    int sw = 1;
    while (sw < wm_shifts(D, L) && sw < WM_CORR_THREADS) sw *= 2;
    return sw;
}
constexpr int wm_corr_ranges(int D, int L) { return (wm_shifts(D, L) + wm_corr_shifts(D, L) - 1) / wm_corr_shifts(D, L); }
// the packed signs: one bit a chip for q < chips + shifts, in 32-bit words with two words to spare
constexpr long long wm_sign_words(long long N, int L, int D) {
    return (wm_chips_padded(N, L) + (long long)wm_corr_ranges(D, L) * wm_corr_shifts(D, L) + 31) / 32 + 2;
}
// LDS of a correlation workgroup: P x 128 int64 sums, a tile of int16 chip sums, its sign words
constexpr size_t wm_corr_lds(int P) {
    return (size_t)P * WM_CORR_THREADS * 8 + (size_t)WM_CORR_TILE * 2 + (size_t)((WM_CORR_TILE + WM_CORR_THREADS) / 32 + 2) * 4;
}

// ---- the plain restatement for one row (the check program)
inline void wm_envelope(const float* x, long long n, float* e /* [n] */) {
    const long long nb = wm_blocks(n);
    for (long long i = 0; i < n; ++i) {
        const long long k = i / WM_BLOCK;
        float E[3] = {0.0f, 0.0f, 0.0f};
        for (int o = -1; o <= 1; ++o) {
            const long long kk = k + o;
            if (kk < 0 || kk >= nb) continue;
            for (long long t = kk * WM_BLOCK; t < n && t < (kk + 1) * WM_BLOCK; ++t) E[o + 1] = fmaxf(E[o + 1], wm_magnitude(x[t]));
        }
        e[i] = wm_min3(E[0], E[1], E[2]);
    }
}
// chip sum i of phase f
inline int wm_chip_sum(const int* v, long long n, int L, int f, long long i) {
    int a = 0;
    for (int t = 0; t < L; ++t) {
        const long long s = i * L + t - f;
        if (s >= 0 && s < n) a += t < L / 2 ? v[s] : -v[s];
    }
    return a;
}

// ---- the argument checks
inline std::string wm_range(const char* what, long long v, long long lo, long long hi) {
    if (v >= lo && v <= hi) return std::string();
    return std::string(what) + " " + std::to_string(v) + " is not in " + std::to_string(lo) + " .. " + std::to_string(hi);
}
inline std::string wm_params_check(const WmParams& w) {
    std::string bad = wm_range("payload_bits =", w.payload_bits, 1, WM_BITS_MAX);
    if (bad.empty()) bad = wm_range("chip =", w.chip, WM_CHIP_MIN, WM_CHIP_MAX);
    if (bad.empty() && (w.chip & 1)) bad = "chip = " + std::to_string(w.chip) + " is not even";
    if (bad.empty()) bad = wm_range("chips_per_symbol =", w.chips_per_symbol, 1, WM_SYMBOL_MAX);
    if (bad.empty() && !(w.strength >= 0.0 && w.strength <= WM_STRENGTH_MAX)) bad = "strength is not in 0 .. 0.25";
    return bad;
}
// The checks of tts_watermark_embed in the order the header lists them; wav, out: the addresses.  Empty: the call is legal.
inline std::string wm_embed_check(uintptr_t wav, uintptr_t out, int B, int N, const int32_t* n_samples, const WmParams* w) {
    if (!wav || !out || !w) return "a NULL pointer (wav, out and params are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N, 0);
    if (bad.empty()) bad = wm_params_check(*w);
    if (!bad.empty()) return bad;
    return in_out_refusal(wav, out, B, N);
}
// ... and of tts_watermark_detect
inline std::string wm_detect_check(uintptr_t wav, uintptr_t records, int B, int N, const int32_t* n_samples, const WmParams* w, int D,
                                   uintptr_t scores, uintptr_t sums) {
    if (!wav || !records || !w) return "a NULL pointer (wav, records and params are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    std::string bad = lengths_refusal("n_samples", n_samples, B, "N", N, 0);
    if (bad.empty()) bad = wm_params_check(*w);
    if (bad.empty()) bad = wm_range("D =", D, 1, WM_MAX_OFFSETS);
    if (!bad.empty()) return bad;
    if (wav & 3) return "wav must be 4-byte aligned";
    if ((records | scores | sums) & 7) return "records, scores and sums must be 8-byte aligned";
    return std::string();
}

}  // namespace tts
