// The delivery encoder, host side: the formats, the per-sample function every side runs (kernel, tests/encode_check.cpp; the numpy
// restatement is tests/encode_oracle.py), the G.711 segment search, the tile arithmetic of the kernel and the argument checks of
// tts_encode and tts_set_output.  Plain C++ (no HIP, no handle): encode.hip includes it, and tests/encode_check.cpp compiles it alone.
//
// Sample i of row b, for i < n[b]:
//   v = (double)x * Q                  Q = 128 (U8), 32768 (S16, mu-law, A-law): exact
//   d = 0, or with TPDF dither         k = seed + 0x9E3779B97F4A7C15 * (((uint64)b << 32 | i) + 1), z = splitmix64's finaliser of k,
//                                      d = ((double)(z >> 32) - (double)(z & 0xFFFFFFFF)) * 2^-32: exact, triangular on (-1, 1)
//   q = rint(v + d)                    one rounded sum, then ties to even; NaN -> 0 and counted; outside [-Q, Q - 1] -> saturated and
//                                      counted
//   code                               S16: q.  U8: q + 128.  mu-law / A-law: ITU-T G.711 from the 16-bit q, the CCITT / Sun g711.c
//                                      arithmetic (mu-law from q >> 2, clip 8159, bias 33; A-law from q >> 3, negative magnitudes
//                                      -v - 1)
// Samples i >= n[b] are the format's code for zero and count nowhere.
#pragma once
#include "resample_plan.h"
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#ifdef __HIPCC__
#define ENC_HD __host__ __device__ inline
#else
#define ENC_HD inline
#endif

namespace tts {

// (the values of TTS_FMT_* and TTS_DITHER_* in include/sstts_hip.h)
constexpr int ENC_F32 = 0, ENC_S16 = 1, ENC_U8 = 2, ENC_MULAW = 3, ENC_ALAW = 4;
constexpr int ENC_DITHER_NONE = 0, ENC_DITHER_TPDF = 1;
constexpr int ENC_UTTS = 64;                        // rows per launch: their lengths travel by value
constexpr int ENC_LANES = 256;
constexpr int ENC_GROUP = 4;                        // samples of a packed store: one 16-byte load, 8 or 4 bytes of codes
constexpr int ENC_ROUNDS = 4;                      // groups a lane takes, ENC_LANES groups apart
constexpr int ENC_TILE = ENC_ROUNDS * ENC_LANES * ENC_GROUP;   // samples of a row one workgroup takes

constexpr bool enc_format_known(int format) { return format >= ENC_F32 && format <= ENC_ALAW; }
constexpr bool enc_format_coded(int format) { return format >= ENC_S16 && format <= ENC_ALAW; }
constexpr int enc_width(int format) { return format == ENC_F32 ? 4 : format == ENC_S16 ? 2 : enc_format_coded(format) ? 1 : -1; }
constexpr int enc_q(int format) { return format == ENC_U8 ? 128 : 32768; }
constexpr long long enc_tiles(long long N) { return (N + ENC_TILE - 1) / ENC_TILE; }

// The tile of a workgroup is samples [lo, hi) of its row.  Packed stores need the code's address aligned to the store: the samples in
// front of the first aligned group (at most 3) and behind the last whole group (at most 3) go one by one.  `elem`: the index of the
// tile's first code counted in codes from address 0 (the address over the code's width).
constexpr int enc_head(unsigned long long elem) { return (int)((ENC_GROUP - (elem & (ENC_GROUP - 1))) & (ENC_GROUP - 1)); }

// The number of significant bits of v >= 0 (0 for 0)
ENC_HD int enc_bits(int v) { return v < 1 ? 0 : 32 - __builtin_clz((unsigned)v); }
// The G.711 segment search: the first i of 0 .. 7 with v <= (1 << (first_bits + i)) - 1, 8 if there is none.  The tables of g711.c
// are 0x3F, 0x7F .. 0x1FFF (mu-law, first_bits 6) and 0x1F, 0x3F .. 0xFFF (A-law, first_bits 5).
ENC_HD int enc_segment(int v, int first_bits) {
    const int s = enc_bits(v) - first_bits;
    return s < 0 ? 0 : s > 8 ? 8 : s;
}

// linear2ulaw of g711.c on the 16-bit q
ENC_HD unsigned enc_mulaw(int q) {
    int v = q >> 2;
    const unsigned mask = v < 0 ? 0x7Fu : 0xFFu;
    if (v < 0) v = -v;
    if (v > 8159) v = 8159;
    v += 33;
    const int seg = enc_segment(v, 6);
    if (seg >= 8) return 0x7Fu ^ mask;
    return (((unsigned)seg << 4) | (((unsigned)v >> (seg + 1)) & 0xFu)) ^ mask;
}

// linear2alaw of g711.c on the 16-bit q
ENC_HD unsigned enc_alaw(int q) {
    int v = q >> 3;
    const unsigned mask = v >= 0 ? 0xD5u : 0x55u;
    if (v < 0) v = -v - 1;
    const int seg = enc_segment(v, 5);
    if (seg >= 8) return 0x7Fu ^ mask;
    return (((unsigned)seg << 4) | (((unsigned)v >> (seg < 2 ? 1 : seg)) & 0xFu)) ^ mask;
}

// the code of the saturated integer q
ENC_HD unsigned enc_code(int format, int q) {
    return format == ENC_S16 ? (unsigned)q & 0xFFFFu : format == ENC_U8 ? (unsigned)(q + 128) : format == ENC_MULAW ? enc_mulaw(q) : enc_alaw(q);
}
// digital silence: the code of q = 0
constexpr unsigned enc_silence(int format) { return format == ENC_S16 ? 0u : format == ENC_U8 ? 0x80u : format == ENC_MULAW ? 0xFFu : 0xD5u; }

// the TPDF dither of sample i of row b
ENC_HD double enc_dither(uint64_t seed, uint32_t b, uint32_t i) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)b << 32) | (uint64_t)i) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(uint32_t)(z >> 32) - (double)(uint32_t)(z & 0xFFFFFFFFull)) * (1.0 / 4294967296.0);
}

// What a sample adds to its row's record
struct EncCount {
    int clipped = 0, nans = 0, peak = 0;
};

// The saturated integer of a sample: x times Q plus the dither d, rounded to the nearest integer, ties to even
ENC_HD int enc_quantise(float x, int Q, double d, EncCount& c) {
    const double v = (double)x * (double)Q;
    const double r = rint(v + d);
    if (r != r) {
        ++c.nans;
        return 0;
    }
    int q;
    if (r < (double)-Q) {
        q = -Q;
        ++c.clipped;
    } else if (r > (double)(Q - 1)) {
        q = Q - 1;
        ++c.clipped;
    } else {
        q = (int)r;
    }
    const int a = q < 0 ? -q : q;
    if (a > c.peak) c.peak = a;
    return q;
}

// sample i of row b as its code
ENC_HD unsigned enc_sample(float x, int format, int dither, uint64_t seed, uint32_t b, uint32_t i, EncCount& c) {
    const double d = dither == ENC_DITHER_TPDF ? enc_dither(seed, b, i) : 0.0;
    return enc_code(format, enc_quantise(x, enc_q(format), d, c));
}

// The checks of tts_encode, in the order the header lists them; an empty string: the call is legal.  n_samples: host lengths or null
// (all N) -- a row may hold no sample at all.
inline std::string encode_check(bool have_ptrs, int B, int N, const int32_t* n_samples, int format, int dither) {
    if (!have_ptrs) return "a NULL pointer (wav and out are required)";
    if (B < 1 || N < 1) return "need B, N >= 1";
    if (!enc_format_known(format)) return "the format " + std::to_string(format) + " is not one of TTS_FMT_*";
    if (format == ENC_F32) return "TTS_FMT_F32 is no encoding: the rows are float32 already";
    if (dither != ENC_DITHER_NONE && dither != ENC_DITHER_TPDF) return "the dither " + std::to_string(dither) + " is not one of TTS_DITHER_*";
    return lengths_refusal("n_samples", n_samples, B, "N", N, 0);
}

// The checks of tts_set_output; an empty string: legal.  *on: whether the setting changes anything of a call -- an encoding, or two
// different rates; (TTS_FMT_F32, any dither, r, r) is off.
inline std::string output_check(int format, int dither, int rate_in, int rate_out, bool* on) {
    if (!enc_format_known(format)) return "the format " + std::to_string(format) + " is not one of TTS_FMT_*";
    if (format != ENC_F32 && dither != ENC_DITHER_NONE && dither != ENC_DITHER_TPDF)
        return "the dither " + std::to_string(dither) + " is not one of TTS_DITHER_*";
    if (rate_in != rate_out) {
        if (rate_in < 1 || rate_out < 1) return "the rates must be positive";
        if (!resample_ratio_ok((double)rate_out / (double)rate_in))
            return "the ratio rate_out / rate_in = " + std::to_string(rate_out) + " / " + std::to_string(rate_in) + " must lie in [0.25, 4]";
    }
    if (on) *on = format != ENC_F32 || rate_in != rate_out;
    return std::string();
}

}  // namespace tts
