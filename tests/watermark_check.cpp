// Stand-alone check of the host side of the watermark (csrc/watermark_plan.h compiled as plain C++, no GPU, no library): prints the
// constants, the workspace sizes of a table of shapes, the hash and the carrier at a list of positions, a short row's envelope, its
// marked samples, its v and its chip sums at every phase, and what tts_watermark_embed, tts_watermark_detect and tts_set_watermark
// answer to a list of argument sets, for tests/test_watermark_program.py to hold against tests/watermark_oracle.py.  Integers travel
// as they are, doubles and floats as hex floats.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "watermark_plan.h"
#include "check_expect.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

static const WmParams kKnown = {0x0123456789ABCDEFull, 0xB6u, 8, 6, 5, 0.03125};

static float sample(int i) { return (float)((i * 37) % 101 - 50) / 64.0f * (i % 700 < 350 ? 1.0f : 0.03125f); }

// 0: legal, 1: TTS_ERR_INVALID
static int embed_answer(uintptr_t wav, uintptr_t out, int B, int N, const std::vector<int32_t>* n, const WmParams* p) {
    g_why = wm_embed_check(wav, out, B, N, n ? n->data() : nullptr, p);
    return g_why.empty() ? 0 : 1;
}
static int detect_answer(uintptr_t wav, uintptr_t rec, int B, int N, const std::vector<int32_t>* n, const WmParams* p, int D, uintptr_t scores = 0,
                         uintptr_t sums = 0) {
    g_why = wm_detect_check(wav, rec, B, N, n ? n->data() : nullptr, p, D, scores, sums);
    return g_why.empty() ? 0 : 1;
}

int main() {
    std::printf("consts %d %d %d %d %d %a %d %d %d %d %d %d\n", WM_BLOCK, WM_BITS_MAX, WM_CHIP_MIN, WM_CHIP_MAX, WM_SYMBOL_MAX, WM_STRENGTH_MAX,
                WM_MAX_OFFSETS, WM_UTTS, WM_TILE, WM_CORR_TILE, WM_CORR_THREADS, WM_V_MAX);
    for (long long n : {1LL, 63LL, 64LL, 65LL, 4096LL, 4097LL, 275000LL, 2147483647LL})
        for (int L : {2, 8, 16})
            for (int D : {1, 9, 64, 1024, 4096})
                std::printf("ws %lld %d %d %lld %lld %lld %lld %lld %d %d %d %lld\n", n, L, D, wm_blocks(n), wm_tiles(n), wm_chips(n, L), wm_corr_tiles(n, L),
                            wm_chips_padded(n, L), wm_shifts(D, L), wm_corr_shifts(D, L), wm_corr_ranges(D, L), wm_sign_words(n, L, D));
    for (int P : {1, 16, 32}) std::printf("lds %d %zu\n", P, wm_corr_lds(P));
    expect(wm_corr_lds(WM_BITS_MAX) <= 64 * 1024, "the correlation's LDS fits the default limit");
    expect(sizeof(WmParams) == 32, "the parameters are 32 bytes");

    for (uint64_t key : {0ull, 1ull, 0x0123456789ABCDEFull, ~0ull})
        for (uint64_t q : {0ull, 1ull, 2ull, 1000003ull, (1ull << 32) + 5ull})
            std::printf("hash %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", key, q, wm_hash(key, q), wm_chip_negative(key, q));

    const int n = 700;
    for (int i = 0; i < n; ++i) {
        const int s = wm_carrier(kKnown, (uint64_t)i);
        expect(s == wm_carrier_u32(kKnown, (uint32_t)i), "both forms of the carrier agree");
        std::printf("carrier %d %d\n", i, s);
    }
    for (uint64_t p : {(1ull << 31) - 1, (1ull << 32) - 1}) expect(wm_carrier(kKnown, p) == wm_carrier_u32(kKnown, (uint32_t)p), "... up to 2^32 - 1");
    std::printf("carrier %" PRIu64 " %d\n", (1ull << 40) + 12345ull, wm_carrier(kKnown, (1ull << 40) + 12345ull));

    // a row: seams of blocks, a short last block, a loud and a quiet stretch, the special values
    {
        std::vector<float> x(n), e(n);
        for (int i = 0; i < n; ++i) x[i] = sample(i);
        x[100] = std::numeric_limits<float>::quiet_NaN();
        x[101] = std::numeric_limits<float>::infinity();
        x[102] = -0.0f;
        x[300] = 1e-45f;
        wm_envelope(x.data(), n, e.data());
        std::vector<int> v(n);
        for (int i = 0; i < n; ++i) {
            bool m = false;
            const float y = wm_mark(x[i], e[i], kKnown.strength, wm_carrier(kKnown, (uint64_t)i), &m);
            v[i] = wm_v(x[i], e[i]);
            std::printf("row %d %a %a %d %d\n", i, (double)e[i], (double)y, (int)m, v[i]);
            if (!m) expect(std::memcmp(&x[i], &y, 4) == 0, "an unmarked sample is its own bits");
        }
        bool m = true;
        expect(std::isnan(wm_mark(x[100], 0.5f, 0.25, 1, &m)) && !m, "a NaN is not marked");
        expect(std::isinf(wm_mark(x[101], 0.5f, 0.25, -1, &m)) && !m, "nor is an infinity");
        expect(wm_v(x[100], 0.5f) == 0 && wm_v(x[101], 0.5f) == 0 && wm_v(0.3f, 0.0f) == 0, "v is 0 for a sample that is not finite and under no envelope");
        expect(wm_v(1.0f, 0.25f) == 127 && wm_v(-1.0f, 0.25f) == -127, "v saturates");
        expect(wm_v(0.5f / 64.0f, 1.0f) == 0 && wm_v(1.5f / 64.0f, 1.0f) == 2 && wm_v(-2.5f / 64.0f, 1.0f) == -2, "ties go to even");
        for (int L : {2, 6, 16})
            for (int f = 0; f < L; ++f)
                for (long long i = 0; i < wm_chips(n, L); ++i) std::printf("chip %d %d %lld %d\n", L, f, i, wm_chip_sum(v.data(), n, L, f, i));
    }

    // the parameters
    {
        struct { const char* name; WmParams p; } sets[] = {
            {"legal", kKnown}, {"legal_lo", {0, 0, 1, 2, 1, 0.0}}, {"legal_hi", {~0ull, ~0u, 32, 16, 65536, 0.25}},
            {"P0", {1, 1, 0, 8, 64, 0.02}}, {"P33", {1, 1, 33, 8, 64, 0.02}}, {"L0", {1, 1, 16, 0, 64, 0.02}}, {"L7", {1, 1, 16, 7, 64, 0.02}},
            {"L18", {1, 1, 16, 18, 64, 0.02}}, {"C0", {1, 1, 16, 8, 0, 0.02}}, {"C65537", {1, 1, 16, 8, 65537, 0.02}},
            {"G-", {1, 1, 16, 8, 64, -0.01}}, {"G+", {1, 1, 16, 8, 64, 0.2500001}}, {"Gnan", {1, 1, 16, 8, 64, std::numeric_limits<double>::quiet_NaN()}},
            {"order_P_before_L", {1, 1, 0, 7, 0, -1.0}},
        };
        for (auto& s : sets) {
            const std::string why = wm_params_check(s.p);
            std::printf("refuse %s %d\n", s.name, why.empty() ? 0 : 1);
            if (!std::strcmp(s.name, "order_P_before_L")) expect(why.find("payload_bits") == 0, "the parameters are refused in their order");
        }
    }
    // the calls
    {
        const uintptr_t a = 0x10000, o = 0x90000, r = 0x20000;
        const int B = 2, N = 5000;
        const std::vector<int32_t> ok{0, 5000}, lo{5000, -1}, hi{5000, 5001};
        WmParams bad = kKnown;
        bad.chip = 5;
        std::printf("check legal %d\n", embed_answer(a, o, B, N, nullptr, &kKnown));
        std::printf("check legal_lengths %d\n", embed_answer(a, o, B, N, &ok, &kKnown));
        std::printf("check legal_in_place %d\n", embed_answer(a, a, B, N, &ok, &kKnown));
        std::printf("check legal_adjacent %d\n", embed_answer(a, a + (uintptr_t)B * N * 4, B, N, &ok, &kKnown));
        std::printf("check wav %d\n", embed_answer(0, o, B, N, nullptr, &kKnown));
        std::printf("check out %d\n", embed_answer(a, 0, B, N, nullptr, &kKnown));
        std::printf("check params %d\n", embed_answer(a, o, B, N, nullptr, nullptr));
        std::printf("check B %d\n", embed_answer(a, o, 0, N, nullptr, &kKnown));
        std::printf("check N %d\n", embed_answer(a, o, B, 0, nullptr, &kKnown));
        std::printf("check n_lo %d\n", embed_answer(a, o, B, N, &lo, &kKnown));
        std::printf("msg n_samples=-1 %s\n", g_why.c_str());
        std::printf("check n_hi %d\n", embed_answer(a, o, B, N, &hi, &kKnown));
        std::printf("msg n_samples=5001 %s\n", g_why.c_str());
        std::printf("check chip %d\n", embed_answer(a, o, B, N, nullptr, &bad));
        std::printf("check lengths_before_params %d\n", embed_answer(a, o, B, N, &hi, &bad));
        expect(g_why.find("n_samples") == 0, "the lengths are refused ahead of the parameters");
        std::printf("check align %d\n", embed_answer(a + 2, o, B, N, nullptr, &kKnown));
        std::printf("check align_out %d\n", embed_answer(a, o + 1, B, N, nullptr, &kKnown));
        std::printf("check overlap %d\n", embed_answer(a, a + 4, B, N, nullptr, &kKnown));
        std::printf("check overlap_behind %d\n", embed_answer(a + 4, a, B, N, nullptr, &kKnown));
        std::printf("check d_legal %d\n", detect_answer(a, r, B, N, &ok, &kKnown, 64, o, o + 8));
        std::printf("check d_legal_D1 %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 1));
        std::printf("check d_legal_D4096 %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 4096));
        std::printf("check d_wav %d\n", detect_answer(0, r, B, N, nullptr, &kKnown, 64));
        std::printf("check d_records %d\n", detect_answer(a, 0, B, N, nullptr, &kKnown, 64));
        std::printf("check d_params %d\n", detect_answer(a, r, B, N, nullptr, nullptr, 64));
        std::printf("check d_B %d\n", detect_answer(a, r, 0, N, nullptr, &kKnown, 64));
        std::printf("check d_n_hi %d\n", detect_answer(a, r, B, N, &hi, &kKnown, 64));
        std::printf("check d_chip %d\n", detect_answer(a, r, B, N, nullptr, &bad, 64));
        std::printf("check d_D0 %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 0));
        std::printf("check d_D4097 %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 4097));
        std::printf("check d_params_before_D %d\n", detect_answer(a, r, B, N, nullptr, &bad, 0));
        expect(g_why.find("chip") == 0, "the parameters are refused ahead of D");
        std::printf("check d_align %d\n", detect_answer(a + 2, r, B, N, nullptr, &kKnown, 64));
        std::printf("check d_align_records %d\n", detect_answer(a, r + 4, B, N, nullptr, &kKnown, 64));
        std::printf("check d_align_scores %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 64, o + 4));
        std::printf("check d_align_sums %d\n", detect_answer(a, r, B, N, nullptr, &kKnown, 64, o, o + 12));
    }
    return exit_status();
}
