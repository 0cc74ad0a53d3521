// Stand-alone check of the Griffin-Lim run planner (csrc/gl_plan.hip compiled as host C++, no GPU, no library): over a grid of
// batches the runs must tile every utterance exactly, stay inside it, and carry slot words that agree with slots_per_utt.
// Built and run by tests/test_gl_plan_program.py, with -fsanitize=address,undefined where the compiler has the runtimes.
#include "gl_plan.h"
#include "check_expect.h"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

static int g_cases = 0;

static void fail(const std::string& what, const std::string& why) {
    if (++g_failures <= 20) std::fprintf(stderr, "FAIL %s: %s\n", what.c_str(), why.c_str());
}

// lens: frames per utterance; uniform: plan with lens == null and T = lens[0]
static std::vector<GlItem> check_case(const std::vector<int>& lens, bool uniform, int win, int hop, int workers, int n_stage, int force_runs,
                                      int force_run_len) {
    const int B = (int)lens.size();
    const int T_max = *std::max_element(lens.begin(), lens.end());
    char tag[200];
    std::snprintf(tag, sizeof tag, "%s B=%d T_max=%d first=%d %d/%d workers=%d n_stage=%d runs=%d run_len=%d", uniform ? "uniform" : "ragged", B,
                  T_max, lens[0], win, hop, workers, n_stage, force_runs, force_run_len);
    ++g_cases;
    std::vector<GlItem> items;
    int spu = -1, used = -1;
    const int n = gl_plan_items(uniform ? nullptr : lens.data(), uniform ? lens[0] : T_max, B, win, hop, workers, n_stage, force_runs, force_run_len,
                                &items, &spu, &used);
    if (n != (int)items.size() || n < B) fail(tag, "returned count " + std::to_string(n) + " against " + std::to_string(items.size()) + " items");
    if (spu < 1) fail(tag, "slots_per_utt " + std::to_string(spu));
    const bool forced = force_runs >= 1 || force_run_len >= GL_NW;
    if (used < 1 || (!forced && used > workers)) fail(tag, "workers_out " + std::to_string(used));
    // what the library sizes the per-run partials by before a cut is planned (gl_scratch, api_griffin_lim.hip): no planned run is
    // shorter than half a round of the waves
    if (!forced && spu > T_max / (GL_NW / 2) + 1)
        fail(tag, "slots_per_utt " + std::to_string(spu) + " beyond T_max / (GL_NW / 2) + 1 = " + std::to_string(T_max / (GL_NW / 2) + 1));
    std::vector<std::vector<GlItem>> of((size_t)B);
    for (const GlItem& it : items) {
        if (it.b < 0 || it.b >= B) { fail(tag, "utterance " + std::to_string(it.b)); return items; }
        // no run leaves its utterance
        if (it.len < 1 || it.t0 < 0 || it.t0 + it.len > lens[it.b])
            fail(tag, "run [" + std::to_string(it.t0) + ", +" + std::to_string(it.len) + ") leaves utterance " + std::to_string(it.b) + " of " +
                          std::to_string(lens[it.b]) + " frames");
        of[it.b].push_back(it);
    }
    int most = 0;
    for (int b = 0; b < B; ++b) {
        auto& r = of[b];
        std::sort(r.begin(), r.end(), [](const GlItem& x, const GlItem& y) { return x.t0 < y.t0; });
        // the runs tile [0, n_frames[b]) exactly
        int t = 0;
        for (const GlItem& it : r) {
            if (it.t0 != t) fail(tag, "utterance " + std::to_string(b) + ": run starts at " + std::to_string(it.t0) + ", expected " + std::to_string(t));
            t = it.t0 + it.len;
        }
        if (t != lens[b]) fail(tag, "utterance " + std::to_string(b) + ": runs end at " + std::to_string(t) + " of " + std::to_string(lens[b]));
        most = std::max(most, (int)r.size());
    }
    // slot words: the low half is the run's ordinal in its utterance; the high half, on the utterance's last run alone, is the
    // number of slots up to slots_per_utt that no run of the utterance writes; slots_per_utt is the most runs of any utterance
    if (spu != most) fail(tag, "slots_per_utt " + std::to_string(spu) + ", most runs of an utterance " + std::to_string(most));
    for (int b = 0; b < B; ++b)
        for (size_t k = 0; k < of[b].size(); ++k) {
            const int ord = of[b][k].slot & 0xffff, pad = of[b][k].slot >> 16;
            const int want_pad = k + 1 == of[b].size() ? spu - (int)of[b].size() : 0;
            if (ord != (int)k || pad != want_pad)
                fail(tag, "utterance " + std::to_string(b) + " run " + std::to_string(k) + ": slot word " + std::to_string(ord) + " | " +
                              std::to_string(pad) + " << 16, expected " + std::to_string(k) + " | " + std::to_string(want_pad) + " << 16");
        }
    return items;
}

int main() {
    const int pairs[2][2] = {{1102, 275}, {800, 200}};
    const int worker_counts[3] = {16, 224, 256};
    const int batches[3] = {1, 3, 64};
    const int forced[4][2] = {{0, 0}, {3, 0}, {0, 16}, {1, 0}};   // {runs, run_len}
    for (const auto& wh : pairs) {
        const int win = wh[0], hop = wh[1];
        // geometry: one helper for the ring and the planner; the rings of every launch form fit the budget
        const GlStreamGeom g = gl_stream_geom(win, hop);
        if (g.halo != (win + hop - 1) / hop - 1 || g.lag < g.halo || g.lag > g.halo + 1 || g.S % 128 || g.acc_len != g.S - hop || g.wpad != (NFFT - win) / 2)
            fail("geometry", std::to_string(win) + "/" + std::to_string(hop));
        for (int n_stage = 1; n_stage <= 3; ++n_stage) {
            const int R = gl_stream_ring_frames(win, hop, n_stage);
            if (R < GL_NW || gl_stream_lds_bytes(win, hop, R, n_stage) > (size_t)GL_LDS_BUDGET)
                fail("ring", std::to_string(win) + "/" + std::to_string(hop) + " n_stage " + std::to_string(n_stage) + ": " + std::to_string(R) + " frames");
        }
        // the shortest legal utterance: hop (T - 1) > n_fft / 2
        const int T_short = MH / hop + 2;
        for (int workers : worker_counts)
            for (int B : batches)
                for (const auto& f : forced)
                    for (int n_stage = 1; n_stage <= 3; n_stage += 2) {
                        for (int T : {T_short, 37, 1000}) check_case(std::vector<int>((size_t)B, T), true, win, hop, workers, n_stage, f[0], f[1]);
                        // ragged: the shortest legal utterance first, one of 1000 frames, the rest drawn between them
                        std::vector<int> lens((size_t)B);
                        unsigned x = 12345u + (unsigned)(B * 131 + workers);
                        for (int b = 0; b < B; ++b) {
                            x = x * 1664525u + 1013904223u;
                            lens[b] = T_short + (int)((x >> 8) % (unsigned)(1000 - T_short + 1));
                        }
                        lens[0] = T_short;
                        if (B > 1) lens[B - 1] = 1000;
                        check_case(lens, false, win, hop, workers, n_stage, f[0], f[1]);
                        // short utterances only (more workgroups than rounds of the waves)
                        for (int b = 0; b < B; ++b) lens[b] = T_short + b % 21;
                        check_case(lens, false, win, hop, workers, n_stage, f[0], f[1]);
                        // lengths that are all equal: the uniform cut, item for item
                        const std::vector<int> same((size_t)B, 37);
                        const std::vector<GlItem> u = check_case(same, true, win, hop, workers, n_stage, f[0], f[1]);
                        const std::vector<GlItem> r = check_case(same, false, win, hop, workers, n_stage, f[0], f[1]);
                        bool eq = u.size() == r.size();
                        for (size_t k = 0; eq && k < u.size(); ++k)
                            eq = u[k].b == r[k].b && u[k].t0 == r[k].t0 && u[k].len == r[k].len && u[k].slot == r[k].slot;
                        if (!eq) fail("equal lengths", "the ragged call's table differs from the uniform one");
                    }
    }
    // the window images: zero outside the window, the analysis set scaled by 1 / n_fft
    {
        const int win = 800, hop = 200, T = 9;
        std::vector<float> w((size_t)win, 1.0f), rw((size_t)NFFT + hop * (T - 1), 2.0f), out(2 * 16 * 2 * 64, -1.0f);
        gl_build_wlane(w.data(), rw.data(), win, hop, T, out.data());
        const int wpad = gl_stream_geom(win, hop).wpad;
        for (int lane = 0; lane < 64; ++lane)
            for (int c = 0; c < 16; ++c)
                for (int e = 0; e < 2; ++e) {
                    const int nw = 2 * (lane + 64 * c) + e - wpad;
                    const float a = nw >= 0 && nw < win ? 1.0f / NFFT : 0.f;
                    if (out[(0 * 64 + lane) * 32 + 2 * c + e] != a || out[(1 * 64 + lane) * 32 + 2 * c + e] != 2.0f * a) fail("wlane", "image");
                }
    }
    std::printf("gl_plan_check: %d cases, %d failures\n", g_cases, g_failures);
    return exit_status();
}
