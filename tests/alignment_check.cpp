// Stand-alone check of the host side of the attention diagnostics (csrc/alignment_plan.h compiled as plain C++, no GPU, no library):
// prints the cut -- launches and row workgroups -- for a table of batch sizes and step counts, how a wave covers rows of every
// width at every offset from a 16-byte boundary, the keys an argmax is decided by for a list of float patterns, the layout of
// the record, and what tts_alignment_stats and tts_text_lengths answer to a list of argument sets, for
// tests/test_alignment_program.py to hold against the definition.  Built with -fsanitize=address,undefined where the compiler has
// the runtimes.
#include "alignment_plan.h"
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

// 0: legal, 1: TTS_ERR_INVALID
static int answer(bool ptrs, int S, int B, int Ts, const std::vector<int32_t>* n_sent, const std::vector<int32_t>* n_steps) {
    g_why = alignment_check(ptrs, S, B, Ts, n_sent ? n_sent->data() : nullptr, n_steps ? n_steps->data() : nullptr);
    return g_why.empty() ? 0 : 1;
}

static uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

int main() {
    std::printf("consts %d %d %d\n", ALIGN_UTTS, ALIGN_ROWS, ALIGN_LAUNCHES_PER_CHUNK);
    std::printf("record %zu %zu %zu %zu %zu\n", sizeof(tts_alignment_stats_t), offsetof(tts_alignment_stats_t, n_sent),
                offsetof(tts_alignment_stats_t, skipped), offsetof(tts_alignment_stats_t, reserved), offsetof(tts_alignment_stats_t, focus_sum));
    expect(sizeof(AlignCover) == 12, "the cover is three ints");

    for (int B : {1, 2, 63, 64, 65, 128, 129, 1000})
        std::printf("launches %d %d %d\n", B, align_launches(B), length_chunks(B, ALIGN_UTTS));
    for (int S : {1, 2, 3, 4, 5, 40, 200, 1000}) std::printf("blocks %d %d\n", S, align_row_blocks(S));

    // every element of a row exactly once, every float4 on a 16-byte boundary, nothing outside the row
    for (int Ts : {1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 92, 255, 256, 257, 1100}) {
        for (int mis = 0; mis < 4; ++mis) {
            const AlignCover c = align_cover(mis, Ts);
            std::printf("cover %d %d %d %d %d\n", Ts, mis, c.head, c.vecs, c.tail);
            expect(c.head >= 0 && c.head <= 3 && c.vecs >= 0 && c.tail >= 0 && c.tail <= 3, "heads and tails are short");
            expect(c.head + 4 * c.vecs + c.tail == Ts, "the cover is the row");
            expect(c.vecs == 0 || (mis + c.head) % 4 == 0, "the float4s are aligned");
            expect(c.head <= 64 && c.tail <= 64, "one lane per single float");
        }
    }

    // the order of the keys: NaN above +Inf above the finite values above -Inf, the zeros equal, the lower index the larger key
    const float inf = std::numeric_limits<float>::infinity();
    const float values[] = {-inf, -3.0f, -1e-38f, -0.0f, 0.0f, 1e-45f, 0.010978533f, 0.5f, 1.0f, 3e38f, inf};
    const int n_values = (int)(sizeof(values) / sizeof(values[0]));
    for (int i = 0; i < n_values; ++i) {
        std::printf("key %08x %08x\n", bits_of(values[i]), align_value_key(bits_of(values[i])));
        expect(align_value_key(bits_of(values[i])) != 0u, "no key is 0");
        if (i) {
            const bool zeros = values[i] == 0.0f && values[i - 1] == 0.0f;
            expect(zeros ? align_value_key(bits_of(values[i])) == align_value_key(bits_of(values[i - 1]))
                         : align_value_key(bits_of(values[i])) > align_value_key(bits_of(values[i - 1])),
                   "the keys order as the values");
        }
    }
    for (uint32_t nan : {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xffffffffu, 0x7fa00000u}) {
        std::printf("nan %08x %08x\n", nan, align_value_key(nan));
        expect(align_value_key(nan) == 0xffffffffu && align_value_key(nan) > align_value_key(bits_of(inf)), "a NaN is above +Inf");
    }
    expect(align_key(bits_of(0.5f), 3) > align_key(bits_of(0.5f), 4), "a tie goes to the lower index");
    expect(align_key(bits_of(0.5f), 1099) > align_key(bits_of(0.25f), 0), "the value decides first");
    expect(align_key(0x7fc00000u, 9) > align_key(0xffc00001u, 40), "the first NaN wins");
    expect(align_key(0x7fc00000u, 40) > align_key(bits_of(inf), 0), "a NaN wins over +Inf in front of it");
    for (uint32_t idx : {0u, 1u, 63u, 64u, 1099u, 2147483647u}) expect(align_key_index(align_key(bits_of(1.0f), idx)) == (int)idx, "the index comes back");
    expect(align_key(bits_of(-inf), 2147483647u) != 0, "no key is 0");

    const std::vector<int32_t> sent = {92, 1, 60}, steps = {200, 1, 17};
    std::printf("check legal_ragged %d\n", answer(true, 200, 3, 92, &sent, &steps));
    std::printf("check legal_uniform %d\n", answer(true, 200, 3, 92, nullptr, nullptr));
    std::printf("check legal_smallest %d\n", answer(true, 1, 1, 1, nullptr, nullptr));
    std::printf("check legal_largest %d\n", answer(true, 2147483647, 1, 2147483647, nullptr, nullptr));
    std::printf("check null %d\n", answer(false, 200, 3, 92, nullptr, nullptr));
    std::printf("msg null %s\n", g_why.c_str());
    std::printf("check B0 %d\n", answer(true, 200, 0, 92, nullptr, nullptr));
    std::printf("msg B0 %s\n", g_why.c_str());
    std::printf("check Ts0 %d\n", answer(true, 200, 3, 0, nullptr, nullptr));
    std::printf("check S0 %d\n", answer(true, 0, 3, 92, nullptr, nullptr));
    std::printf("check negative %d\n", answer(true, -1, -1, -1, nullptr, nullptr));
    for (int bad : {0, -1, 93}) {
        std::vector<int32_t> l = sent;
        l[1] = bad;
        std::printf("check n_sent=%d %d\n", bad, answer(true, 200, 3, 92, &l, &steps));
        std::printf("msg n_sent=%d %s\n", bad, g_why.c_str());
    }
    for (int bad : {0, -1, 201}) {
        std::vector<int32_t> l = steps;
        l[2] = bad;
        std::printf("check n_steps=%d %d\n", bad, answer(true, 200, 3, 92, &sent, &l));
        std::printf("msg n_steps=%d %s\n", bad, g_why.c_str());
    }
    {   // the sentence lengths are looked at first
        std::vector<int32_t> a = sent, b = steps;
        a[0] = 93;
        b[0] = 0;
        std::printf("check both %d\n", answer(true, 200, 3, 92, &a, &b));
        std::printf("msg both %s\n", g_why.c_str());
    }
    std::printf("text legal %d\n", text_lengths_check(true, 3, 92).empty() ? 0 : 1);
    std::printf("text null %d\n", text_lengths_check(false, 3, 92).empty() ? 0 : 1);
    std::printf("msg text_null %s\n", text_lengths_check(false, 3, 92).c_str());
    std::printf("text B0 %d\n", text_lengths_check(true, 0, 92).empty() ? 0 : 1);
    std::printf("text Ts0 %d\n", text_lengths_check(true, 3, 0).empty() ? 0 : 1);
    std::printf("msg text_B0 %s\n", text_lengths_check(true, 0, 92).c_str());
    return exit_status();
}
