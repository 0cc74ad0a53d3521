// Stand-alone check of the host side of STOI (csrc/stoi_plan.h compiled as plain C++, no GPU, no library): prints the frame and
// segment counts, the groupings of the launches with their LDS bytes, the band table, the window and what tts_stoi answers to a
// list of argument sets, for tests/test_stoi_program.py to hold against tests/stoi_oracle.py.  Built with
// -fsanitize=address,undefined where the compiler has the runtimes.
#include "stoi_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last answer

// 0: legal, 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
static int answer(uintptr_t ref, uintptr_t deg, uintptr_t rec, uintptr_t idx, uintptr_t env, int B, int N, const std::vector<int32_t>* n, int extended) {
    bool unsupported = false;
    const std::string why = stoi_check(ref, deg, rec, idx, env, B, N, n ? n->data() : nullptr, extended, &unsupported);
    g_why = why;
    expect(why.empty() ? !unsupported : true, "unsupported is set with a reason only");
    return why.empty() ? 0 : unsupported ? 2 : 1;
}

int main() {
    std::printf("consts %d %d %d %d %d %d %d %d %d %d %d %d %zu\n", STOI_W, STOI_H, STOI_NFFT, STOI_J, STOI_N, STOI_UTTS, STOI_ENERGY_FRAMES,
                STOI_SCAN_LANES, STOI_MAX_FRAMES, STOI_GROUP, STOI_ENV_LANES, STOI_SEG_CHUNK, STOI_LDS_BUDGET);
    std::printf("lds %zu %zu %zu\n", stoi_energy_lds_bytes(), stoi_env_lds_bytes(), stoi_seg_lds_bytes());
    expect(stoi_energy_lds_bytes() <= STOI_LDS_BUDGET && stoi_env_lds_bytes() <= STOI_LDS_BUDGET && stoi_seg_lds_bytes() <= STOI_LDS_BUDGET,
           "every workgroup's LDS fits the budget");
    // the last sample an energy workgroup stages, and the last a lane reads
    expect((size_t)((STOI_ENERGY_FRAMES + 1) * STOI_H - 1) + STOI_ENERGY_FRAMES < stoi_energy_floats(), "the staged samples fit");
    expect((size_t)(STOI_ENERGY_FRAMES - 1) * (STOI_H + 1) + (STOI_W - 1) + 1 < stoi_energy_floats(), "a lane's walk stays inside");
    expect(STOI_ENV_LANES % 64 == 0 && STOI_SCAN_LANES % 64 == 0, "whole waves");
    expect(STOI_MAX_FRAMES == STOI_SCAN_LANES * STOI_SCAN_RUN, "the scan's lanes and runs cover the most frames");

    for (int n : {1, 127, 255, 256, 257, 383, 384, 385, 511, 512, 20000, 124717, 2147483647})
        std::printf("frames %d %d\n", n, stoi_frames(n));
    for (int kept : {0, 1, 29, 30, 31, 93, 94, 65536}) std::printf("segments %d %d %lld\n", kept, stoi_segments(kept), stoi_compacted(kept));
    for (int frames : {0, 1, 255, 256, 257, 974, 65535, 65536}) {
        const int run = stoi_scan_run(frames);
        std::printf("scan %d %d\n", frames, run);
        expect(run <= STOI_SCAN_RUN && (long long)run * STOI_SCAN_LANES >= frames, "the lanes' runs cover the frames");
    }
    for (int count : {0, 1, 3, 4, 5, 63, 64, 65, 974})
        for (int per : {STOI_GROUP, STOI_SEG_CHUNK, STOI_ENERGY_FRAMES}) std::printf("groups %d %d %d\n", count, per, stoi_groups(count, per));

    int32_t e[STOI_J][2];
    stoi_bands(e);
    for (int j = 0; j < STOI_J; ++j) std::printf("band %d %d %d\n", j, e[j][0], e[j][1]);
    expect(e[0][0] >= 1 && e[STOI_J - 1][1] <= STOI_NFFT / 2, "the bins of the bands and their mirrors lie inside the transform");
    double w[STOI_W];
    stoi_window(w);
    for (int i = 0; i < STOI_W; ++i) std::printf("window %d %.17g\n", i, w[i]);

    // ---- tts_stoi's answers
    const std::vector<int32_t> ls = {5000, 1, 256};
    const uintptr_t p = 4096;
    std::printf("check legal_ragged %d\n", answer(p, p, p, p, p, 3, 5000, &ls, 0));
    std::printf("check legal_uniform %d\n", answer(p, p, p, 0, 0, 3, 5000, nullptr, 1));
    std::printf("check legal_smallest %d\n", answer(p, p, p, 0, 0, 1, 1, nullptr, 0));
    std::printf("check legal_offsets %d\n", answer(p + 4, p + 12, p + 8, p + 4, p + 8, 1, 5000, nullptr, 0));
    const int most = (STOI_MAX_FRAMES - 1) * STOI_H + STOI_W + STOI_H - 1;   // the longest row of STOI_MAX_FRAMES frames
    std::printf("check legal_most_frames %d\n", answer(p, p, p, 0, 0, 1, most, nullptr, 0));
    std::printf("check frames_above %d\n", answer(p, p, p, 0, 0, 1, most + 1, nullptr, 0));
    std::printf("check null_ref %d\n", answer(0, p, p, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check null_deg %d\n", answer(p, 0, p, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check null_records %d\n", answer(p, p, 0, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check B0 %d\n", answer(p, p, p, 0, 0, 0, 5000, nullptr, 0));
    std::printf("check N0 %d\n", answer(p, p, p, 0, 0, 3, 0, nullptr, 0));
    std::printf("check extended2 %d\n", answer(p, p, p, 0, 0, 3, 5000, nullptr, 2));
    std::printf("check extended_negative %d\n", answer(p, p, p, 0, 0, 3, 5000, nullptr, -1));
    std::printf("check ref_misaligned %d\n", answer(p + 2, p, p, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check deg_misaligned %d\n", answer(p, p + 1, p, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check records_misaligned %d\n", answer(p, p, p + 4, 0, 0, 3, 5000, nullptr, 0));
    std::printf("check index_misaligned %d\n", answer(p, p, p, p + 2, 0, 3, 5000, nullptr, 0));
    std::printf("check envelopes_misaligned %d\n", answer(p, p, p, 0, p + 4, 3, 5000, nullptr, 0));
    for (int bad : {0, -1, 5001}) {
        std::vector<int32_t> l = ls;
        l[1] = bad;
        std::printf("check n=%d %d\n", bad, answer(p, p, p, 0, 0, 3, 5000, &l, 0));
        std::printf("msg n_samples=%d %s\n", bad, g_why.c_str());
    }
    return exit_status();
}
