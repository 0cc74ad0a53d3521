// Stand-alone check of the host side of the timing marks (csrc/token_times_plan.h compiled as plain C++, no GPU, no library):
// prints the constants, the layout of the record, the launches for a table of batch sizes, where the directions of a launch
// live and how much LDS it takes, the weight of a list of float patterns, and what tts_token_times answers to a list of argument
// sets, for tests/test_token_times_program.py to hold against the definition.  Built with -fsanitize=address,undefined where the
// compiler has the runtimes.
#include "token_times_plan.h"
#include "../include/sstts_hip.h"
#include "check_expect.h"
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// 0: legal, 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
static int answer(bool ptrs, int S, int B, int Ts, const std::vector<int32_t>* n_sent, const std::vector<int32_t>* n_steps, int J) {
    g_why = token_times_check(ptrs, S, B, Ts, n_sent ? n_sent->data() : nullptr, n_steps ? n_steps->data() : nullptr, J);
    if (!g_why.empty()) return 1;
    g_why = token_times_unsupported(Ts);
    return g_why.empty() ? 0 : 2;
}

static uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

int main() {
    std::printf("consts %d %d %d %d %d %d %zu\n", TT_UTTS, TT_THREADS, TT_PASSES, TT_MAX_TOKENS, TT_MAX_JUMP, TT_LAUNCHES_PER_CHUNK,
                TT_DIR_LDS_BYTES);
    std::printf("record %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tts_token_times_stats_t), offsetof(tts_token_times_stats_t, score),
                offsetof(tts_token_times_stats_t, n_sent), offsetof(tts_token_times_stats_t, n_steps), offsetof(tts_token_times_stats_t, last),
                offsetof(tts_token_times_stats_t, jumps), offsetof(tts_token_times_stats_t, skipped), offsetof(tts_token_times_stats_t, agree));
    expect(alignof(tts_token_times_stats_t) == 8, "the record is 8-byte aligned");
    expect(TT_MAX_TOKENS >= 1024, "at least 1024 tokens");
    expect(tt_lds_bytes(1, TT_MAX_TOKENS) <= 65536 && tt_rows_bytes(TT_MAX_TOKENS) + TT_DIR_LDS_BYTES <= 65536, "a workgroup's LDS is 64 KiB");

    for (int B : {1, 2, 63, 64, 65, 128, 129, 1000})
        std::printf("launches %d %d %d\n", B, tt_launches(B), length_chunks(B, TT_UTTS));

    // the directions: in LDS up to TT_DIR_LDS_BYTES, and the LDS of the launch
    for (int S : {1, 2, 64, 130, 200, 1000}) {
        for (int Ts : {1, 64, 100, 130, 252, 253, 300, 1024}) {
            std::printf("dir %d %d %d %zu\n", S, Ts, tt_dir_in_lds(S, Ts) ? 1 : 0, tt_lds_bytes(S, Ts));
            expect(tt_lds_bytes(S, Ts) <= 65536 - 1024, "the launch fits a workgroup's LDS beside the static arrays");
        }
    }
    expect(tt_dir_in_lds(2147483647, 2147483647) == false, "no overflow in the size of the directions");

    // the weight: the bits of a positive element, 0 for a NaN, a zero and a negative; monotone over the positive floats
    const float inf = std::numeric_limits<float>::infinity();
    const float values[] = {-inf, -3.0f, -1e-38f, -1e-45f, -0.0f, 0.0f, 1e-45f, 1e-39f, 0.010978533f, 0.5f, 1.0f, 3e38f, inf};
    const int n_values = (int)(sizeof(values) / sizeof(values[0]));
    for (int i = 0; i < n_values; ++i) {
        std::printf("weight %08x %08x\n", bits_of(values[i]), tt_weight(bits_of(values[i])));
        expect(tt_weight(bits_of(values[i])) == (values[i] > 0.0f ? bits_of(values[i]) : 0u), "the bits where the element is greater than 0");
        if (i) expect(tt_weight(bits_of(values[i])) >= tt_weight(bits_of(values[i - 1])), "the weights order as the values");
    }
    for (uint32_t nan : {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fa00000u}) {
        std::printf("nan %08x %08x\n", nan, tt_weight(nan));
        expect(tt_weight(nan) == 0u, "a NaN weighs nothing");
    }

    const std::vector<int32_t> sent = {92, 1, 60}, steps = {200, 1, 17};
    std::printf("check legal_ragged %d\n", answer(true, 200, 3, 92, &sent, &steps, 4));
    std::printf("check legal_uniform %d\n", answer(true, 200, 3, 92, nullptr, nullptr, 4));
    std::printf("check legal_smallest %d\n", answer(true, 1, 1, 1, nullptr, nullptr, 1));
    std::printf("check legal_largest %d\n", answer(true, 2147483647, 1, TT_MAX_TOKENS, nullptr, nullptr, TT_MAX_JUMP));
    std::printf("check null %d\n", answer(false, 200, 3, 92, nullptr, nullptr, 4));
    std::printf("msg null %s\n", g_why.c_str());
    std::printf("check B0 %d\n", answer(true, 200, 0, 92, nullptr, nullptr, 4));
    std::printf("msg B0 %s\n", g_why.c_str());
    std::printf("check Ts0 %d\n", answer(true, 200, 3, 0, nullptr, nullptr, 4));
    std::printf("check S0 %d\n", answer(true, 0, 3, 92, nullptr, nullptr, 4));
    std::printf("check negative %d\n", answer(true, -1, -1, -1, nullptr, nullptr, 4));
    for (int bad : {0, -1, 93}) {
        std::vector<int32_t> l = sent;
        l[1] = bad;
        std::printf("check n_sent=%d %d\n", bad, answer(true, 200, 3, 92, &l, &steps, 4));
        std::printf("msg n_sent=%d %s\n", bad, g_why.c_str());
    }
    for (int bad : {0, -1, 201}) {
        std::vector<int32_t> l = steps;
        l[2] = bad;
        std::printf("check n_steps=%d %d\n", bad, answer(true, 200, 3, 92, &sent, &l, 4));
        std::printf("msg n_steps=%d %s\n", bad, g_why.c_str());
    }
    for (int bad : {0, -1, 16}) {
        std::printf("check J=%d %d\n", bad, answer(true, 200, 3, 92, &sent, &steps, bad));
        std::printf("msg J=%d %s\n", bad, g_why.c_str());
    }
    {   // the lengths are looked at before the jump, and everything TTS_ERR_INVALID refuses before the size of the table
        std::vector<int32_t> a = sent;
        a[0] = 93;
        std::printf("check lengths_first %d\n", answer(true, 200, 3, 92, &a, &steps, 0));
        std::printf("msg lengths_first %s\n", g_why.c_str());
        std::printf("check invalid_first %d\n", answer(true, 200, 3, TT_MAX_TOKENS + 1, nullptr, nullptr, 0));
        std::printf("msg invalid_first %s\n", g_why.c_str());
    }
    std::printf("check too_wide %d\n", answer(true, 200, 3, TT_MAX_TOKENS + 1, nullptr, nullptr, 4));
    std::printf("msg too_wide %s\n", g_why.c_str());
    return exit_status();
}
