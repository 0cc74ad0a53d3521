// Stand-alone check of a synthesis call's host-side plan (csrc/synth_plan.h compiled as plain C++, no GPU, no library): prints the
// shape and the per-utterance lengths over a grid of settings for tests/test_synth_plan_program.py to hold against the tests'
// oracles, and runs every refusal of the plan once -- alone, and in pairs for their order.  Built with
// -fsanitize=address,undefined where the compiler has the runtimes.
//
// One line per grid point: n_fft hop T rate octaves stopping, then either "R <which refusal, 1 .. 5>" or
// "OK stretch pitch rate rate_s rho Tw Tg min_frames ragged T_model" followed by, per utterance of a batch of three,
// "detected reported gl n_samples keep kept" (-1: the call has no such value).  kept: the samples the resampler leaves in the
// row, min(resampled_valid(its input, rho), its cap).
#include "synth_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

// which refusal, in the order a call meets them; 0: none
static int which(const std::string& why) {
    if (why.empty()) return 0;
    const char* const marks[] = {"hop_length >= 1", "outside [0.25, 4]", "with a pitch", "Griffin-Lim needs at least", "end-of-speech stopping needs"};
    for (int i = 0; i < 5; ++i)
        if (why.find(marks[i]) != std::string::npos) return i + 1;
    return -1;
}

static int refusal(int T, int n_fft, int hop, double s, double octaves, bool stopping) {
    SynthShape shape;
    return which(synth_shape(T, n_fft, hop, s, octaves, stopping, &shape));
}

static void grid_point(int n_fft, int hop, int T, double s, double octaves, bool stopping) {
    SynthShape sh;
    const std::string why = synth_shape(T, n_fft, hop, s, octaves, stopping, &sh);
    std::printf("%d %d %d %.17g %.17g %d ", n_fft, hop, T, s, octaves, stopping ? 1 : 0);
    if (!why.empty()) {
        std::printf("R %d\n", which(why));
        return;
    }
    const int B = 3;
    const std::vector<int32_t> detected = {sh.min_frames, (sh.min_frames + T) / 2, T};
    SynthLengths L;
    L.n_samples.assign(7, 123);   // (what an earlier call left behind must not show)
    synth_lengths(sh, T, hop, B, stopping ? detected.data() : nullptr, &L);
    expect(L.reported.size() == (size_t)B && L.gl.size() == (size_t)B, "B reported and Griffin-Lim lengths");
    expect(L.n_samples.size() == L.keep.size() && L.n_samples.size() == (sh.pitch && stopping ? (size_t)B : 0),
           "the resampler's lengths exist with a pitch and detected lengths alone");
    std::printf("OK %d %d %.17g %.17g %.17g %d %d %d %d %d", sh.stretch ? 1 : 0, sh.pitch ? 1 : 0, sh.rate, sh.rate_s, sh.rho, sh.Tw, sh.Tg,
                sh.min_frames, L.ragged ? 1 : 0, L.T_model);
    for (int b = 0; b < B; ++b) {
        const bool have = !L.n_samples.empty();
        long long kept = -1;
        if (sh.pitch) {   // (as the resampler cuts a row: resample.hip)
            kept = std::min<long long>(resampled_valid(have ? L.n_samples[b] : hop * (sh.Tg - 1), sh.rho), (long long)hop * (sh.Tw - 1));
            if (have) kept = std::min<long long>(kept, L.keep[b]);
        }
        std::printf(" %d %d %d %d %d %lld", stopping ? detected[b] : -1, L.reported[b], L.gl[b], have ? L.n_samples[b] : -1, have ? L.keep[b] : -1, kept);
    }
    std::printf("\n");
}

int main() {
    const int sizes[][2] = {{2048, 275}, {512, 100}};
    const double rates[] = {0.25, 0.8, 1.0, 1.2, 2.5, 4.0};
    const double octaves[] = {-1.0, -1.0 / 3.0, 0.0, 1.0 / 3.0, 1.0};
    for (const auto& nh : sizes)
        for (int T = 4; T <= 48; ++T)
            for (double s : rates)
                for (double o : octaves)
                    for (int stopping = 0; stopping < 2; ++stopping) grid_point(nh[0], nh[1], T, s, o, stopping != 0);

    expect(speech_min_frames(2048, 275) == 5 && speech_min_frames(512, 100) == 4 && speech_min_frames(2048, 2048) == 2, "min_frames: hop (n - 1) > n_fft / 2");
    {   // rate 1.0 and pitch 0: nothing of the call changes, whatever the hop
        SynthShape sh;
        expect(synth_shape(40, 2048, 275, 1.0, 0.0, false, &sh).empty() && !sh.stretch && !sh.pitch && sh.Tw == 40 && sh.Tg == 40 && sh.min_frames == 5,
               "the call as it was");
        expect(synth_shape(40, 2048, 0, 1.0, 0.0, true, &sh).empty() && sh.min_frames == 1 && sh.Tw == 40 && sh.Tg == 40,
               "a hop below 1 is not this plan's to refuse while no rate and no pitch is set");
    }
    // every refusal alone ...
    expect(refusal(40, 2048, 0, 1.2, 0.0, false) == 1 && refusal(40, 2048, -3, 1.0, 0.5, false) == 1, "hop_length < 1 with a rate or a pitch");
    expect(refusal(40, 2048, 275, 2.5, -1.0, false) == 2 && refusal(40, 2048, 275, 0.4, 1.0, false) == 2, "the product outside [0.25, 4]");
    expect(refusal(40, 2048, 275, 2.5, 1.0, false) == 0, "the product, not the pair, is what the stretch is given");
    expect(refusal(15, 2048, 275, 4.0, 1.0, false) == 3, "rows shorter than min_frames with a pitch (ceil(15 / 4) = 4 < 5, though Griffin-Lim's 8 would do)");
    expect(refusal(15, 2048, 275, 4.0, 0.0, false) == 4 && refusal(8, 2048, 275, 1.0, -1.0, false) == 4, "Tg < min_frames");
    expect(refusal(4, 2048, 275, 1.0, 0.0, true) == 5 && refusal(4, 2048, 275, 1.0, 0.0, false) == 0, "T < min_frames with stopping on");
    expect(refusal(4, 2048, 275, 0.25, 0.0, true) == 5, "... also where the stretched call is long enough");
    // ... and two at once, in the order a call meets them
    expect(refusal(40, 2048, 0, 2.5, -1.0, true) == 1, "the hop before the product");
    expect(refusal(4, 2048, 275, 4.0, -1.0, true) == 2, "the product before the rows");
    expect(refusal(4, 2048, 275, 4.0, 1.0, true) == 3, "the rows before Griffin-Lim's frames (1 and 2 frames)");
    expect(refusal(4, 2048, 275, 1.2, 0.0, true) == 4, "Griffin-Lim's frames before stopping's");
    {   // the wording the callers match on
        SynthShape sh;
        expect(synth_shape(40, 2048, 275, 2.5, -1.0, false, &sh).find("pitch") != std::string::npos, "'pitch' in the product's refusal");
        expect(synth_shape(15, 2048, 275, 4.0, 1.0, false, &sh).find("at this speaking rate") != std::string::npos, "the rows' refusal names the rate");
        expect(synth_shape(4, 2048, 275, 1.0, 1.0, false, &sh).find("at this speaking rate") == std::string::npos, "... only where one is set");
    }
    return exit_status();
}
