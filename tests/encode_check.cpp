// Stand-alone check of the host side of the delivery encoder (csrc/encode_plan.h compiled as plain C++, no GPU, no library): prints
// the per-sample function's codes over all 65 536 levels x 4 formats as checksums and at marked levels, the special values, the
// dither at a few (seed, row, sample), the tile arithmetic and what tts_encode and tts_set_output answer to a list of argument
// sets -- for tests/test_encode_program.py to hold against tests/encode_oracle.py -- and holds the segment search to g711.c's
// table search.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "encode_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;

static int answer(bool ptrs, int B, int N, const std::vector<int32_t>* n, int format, int dither) {
    g_why = encode_check(ptrs, B, N, n ? n->data() : nullptr, format, dither);
    return g_why.empty() ? 0 : 1;
}

// prints "output <case> <0: legal, 1: refused> <*on afterwards>"
static void answer_output(const char* name, int format, int dither, int rate_in, int rate_out, bool* on) {
    g_why = output_check(format, dither, rate_in, rate_out, on);
    std::printf("output %s %d %d\n", name, g_why.empty() ? 0 : 1, (int)*on);
}

// g711.c's search(): the first index whose table entry is >= v
static int table_search(int v, const int* table) {
    for (int i = 0; i < 8; ++i)
        if (v <= table[i]) return i;
    return 8;
}

int main() {
    std::printf("consts %d %d %d %d\n", ENC_UTTS, ENC_LANES, ENC_GROUP, ENC_TILE);
    expect(ENC_TILE % (ENC_LANES * ENC_GROUP) == 0, "the lanes take whole rounds of groups");
    for (int f = -1; f <= 5; ++f) std::printf("width %d %d\n", f, enc_width(f));
    for (int f = ENC_S16; f <= ENC_ALAW; ++f) {
        EncCount c;
        std::printf("silence %d %u %u\n", f, enc_silence(f), enc_sample(0.f, f, ENC_DITHER_NONE, 0, 0, 0, c));
    }

    // the segment search against the tables of g711.c, over every value the encoders hand it and beyond
    const int uend[8] = {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF}, aend[8] = {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF};
    bool same = true;
    for (int v = 0; v <= 70000; ++v) same = same && enc_segment(v, 6) == table_search(v, uend) && enc_segment(v, 5) == table_search(v, aend);
    expect(same, "the segment search is g711.c's table search");

    // every 16-bit level x = k / 32768 (exact in float32), undithered: a checksum per format and the codes at every 257th level
    for (int f = ENC_S16; f <= ENC_ALAW; ++f) {
        EncCount c;
        unsigned long long sum = 0;
        std::printf("levels %d", f);
        for (int k = -32768; k <= 32767; ++k) {
            const unsigned code = enc_sample((float)k / 32768.f, f, ENC_DITHER_NONE, 0, 0, (uint32_t)(k + 32768), c);
            sum = sum * 1000003ull + code;
            if ((k + 32768) % 257 == 0) std::printf(" %u", code);
        }
        std::printf("\nlevelsum %d %llu %d %d %d\n", f, sum, c.clipped, c.nans, c.peak);
    }

    // the special values: the saturated integer and what it counts
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float lsb = 1.f / 32768.f;
    const float specials[] = {1.f, -1.f, 0.99999994f, -0.f, 0.f, 1e-45f, -1e-40f, inf, -inf, nan, 3.0e38f, -3.0e38f, 0.5f * lsb, -0.5f * lsb,
                              1.5f * lsb, -1.5f * lsb, 2.5f * lsb, -2.5f * lsb, 32766.5f * lsb, 32767.5f * lsb, -32768.5f * lsb, -32769.5f * lsb,
                              0.25f, -0.75f};
    for (int Q : {32768, 128}) {
        EncCount c;
        std::printf("special %d", Q);
        for (float x : specials) std::printf(" %d", enc_quantise(x, Q, 0.0, c));
        std::printf("\nspecialcount %d %d %d %d\n", Q, c.clipped, c.nans, c.peak);
    }

    // the dither: exact doubles, printed with all their digits
    for (unsigned long long seed : {0ull, 1234ull, 9223372036854775813ull})
        for (uint32_t b : {0u, 1u, 63u})
            for (uint32_t i : {0u, 1u, 4095u, 4096u, 2147483646u}) {
                const double d = enc_dither(seed, b, i);
                expect(d > -1.0 && d < 1.0, "the dither lies inside (-1, 1)");
                std::printf("dither %llu %u %u %.17g\n", seed, b, i, d);
            }
    // ... and a dithered sample is the rounding of one sum
    {
        EncCount c;
        std::printf("dithered");
        for (uint32_t i = 0; i < 16; ++i) std::printf(" %u", enc_sample(0.25f * lsb * (float)i, ENC_S16, ENC_DITHER_TPDF, 1234, 2, i, c) & 0xFFFFu);
        std::printf("\n");
    }

    for (long long n : {1LL, (long long)ENC_TILE - 1, (long long)ENC_TILE, (long long)ENC_TILE + 1, 2147483647LL})
        std::printf("tiles %lld %lld\n", n, enc_tiles(n));
    // the head of a tile: the samples in front of the first code whose index is a multiple of four
    for (unsigned long long e = 0; e < 8; ++e) {
        std::printf("head %llu %d\n", e, enc_head(e));
        expect((e + (unsigned long long)enc_head(e)) % ENC_GROUP == 0 && enc_head(e) < ENC_GROUP, "the head ends at an aligned code");
    }

    const std::vector<int32_t> ls = {0, 1, 5000};
    std::printf("check legal_ragged %d\n", answer(true, 3, 5000, &ls, ENC_S16, ENC_DITHER_TPDF));
    std::printf("check legal_uniform %d\n", answer(true, 3, 5000, nullptr, ENC_ALAW, ENC_DITHER_NONE));
    std::printf("check legal_largest %d\n", answer(true, 1, 2147483647, nullptr, ENC_MULAW, ENC_DITHER_TPDF));
    std::printf("check legal_u8 %d\n", answer(true, 1, 1, nullptr, ENC_U8, ENC_DITHER_NONE));
    std::printf("check null %d\n", answer(false, 3, 5000, nullptr, ENC_S16, 0));
    std::printf("check B0 %d\n", answer(true, 0, 5000, nullptr, ENC_S16, 0));
    std::printf("check N0 %d\n", answer(true, 3, 0, nullptr, ENC_S16, 0));
    std::printf("check f32 %d\n", answer(true, 3, 5000, nullptr, ENC_F32, 0));
    std::printf("msg f32 %s\n", g_why.c_str());
    for (int f : {-1, 5, 100}) std::printf("check format=%d %d\n", f, answer(true, 3, 5000, nullptr, f, 0));
    for (int d : {-1, 2}) std::printf("check dither=%d %d\n", d, answer(true, 3, 5000, nullptr, ENC_S16, d));
    for (int bad : {-1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(true, 3, 5000, &l, ENC_S16, 0));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }

    bool on = true;
    answer_output("legal_off", ENC_F32, 7, 22050, 22050, &on);
    answer_output("legal_off_no_rates", ENC_F32, 0, 0, 0, &on);
    answer_output("legal_pcm16", ENC_S16, ENC_DITHER_TPDF, 0, 0, &on);
    answer_output("legal_mulaw_8k", ENC_MULAW, ENC_DITHER_NONE, 22050, 8000, &on);
    answer_output("legal_f32_half", ENC_F32, 0, 22050, 11025, &on);
    answer_output("legal_quarter", ENC_ALAW, 1, 32000, 8000, &on);
    answer_output("legal_four", ENC_ALAW, 1, 8000, 32000, &on);
    on = true;
    answer_output("format", 5, 0, 0, 0, &on);
    answer_output("dither", ENC_S16, 2, 0, 0, &on);
    answer_output("below_quarter", ENC_S16, 0, 32001, 8000, &on);
    answer_output("above_four", ENC_S16, 0, 8000, 32001, &on);
    answer_output("rate0", ENC_S16, 0, 0, 8000, &on);
    answer_output("rate_negative", ENC_S16, 0, 22050, -8000, &on);
    return exit_status();
}
