// Host side of the streaming Griffin-Lim kernel (gl_stream_kernel, griffin_lim.hip): the constants the kernel and its planner
// share, the ring geometry, the cut of a batch into runs and the per-lane window images.  Plain C++17 -- no HIP type, no
// runtime call -- so that the planner can be compiled and checked without the library (tests/gl_plan_check.cpp).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace tts {

constexpr int NFFT = 2048;               // the streaming kernel's transform: real 2048 points as 1024 complex ones
constexpr int MH = NFFT / 2;
constexpr int GL_NW = 8;                 // waves per workgroup
constexpr int EX_CPLX = 1088;            // complex values of a wave's exchange buffer (fft_wave.h): 64 rows of E2S >= the 1024 bins of the merge pass
constexpr int CT_SWORDS = 16;            // control words of a workgroup, between the exchange buffers and the rings
constexpr int GL_LDS_BUDGET = 160 * 1024;   // dynamic LDS a workgroup may ask for (one workgroup per compute unit)

// One work item of a launch: RUN `len` frames of utterance `b` from frame `t0` on.  Its partial results (mse, peak) go to slot
// (slot & 0xffff) of the utterance; the run with the utterance's last slot carries in slot >> 16 how many slots up to
// slots_per_utt it has to zero (utterances are not all cut into the same number of runs).  The device reads it as an int4.
struct GlItem { int b, t0, len, slot; };

// What the kernel derives from (window, hop): the window's padding inside the transform, halo = ceil(win / hop) - 1, the indices
// a frame's forward transform runs behind its overlap-add, a frame's span in the ring and what earlier indices have written of it
struct GlStreamGeom { int wpad, halo, lag, S, acc_len; };
GlStreamGeom gl_stream_geom(int win, int hop);

// frames an LDS ring holds when n_stage rings share the budget (0: the window / hop pair does not fit)
int gl_stream_ring_frames(int win, int hop, int n_stage = 1);
size_t gl_stream_lds_bytes(int win, int hop, int ring_frames, int n_stage);

// entries per end of an utterance in GlParams::rw_edge: every sample an edge frame's window reaches
inline int gl_rw_edge_len(int n_fft, int win, int hop) { return n_fft + ((win + hop - 1) / hop - 1) * hop; }

// out[2*16*2*64]: set 0 = window[n] / n_fft, set 1 = set 0 * rwss at an interior frame; n = 2*(lane + 64 c) + e
void gl_build_wlane(const float* window, const float* rwss, int win, int hop, int T, float* out);

// The cut of a batch for launches of n_stage iterations on n_workers workgroups, in the order the workgroups draw the items;
// returns their number.  lens[b]: frames of utterance b (null: T in every one).  force_*: gl_plan.hip.
int gl_plan_items(const int* lens, int T, int B, int win, int hop, int n_workers, int n_stage, int force_runs, int force_run_len,
                  std::vector<GlItem>* items, int* slots_per_utt, int* workers_out = nullptr);

// ---- The argument rules of the Griffin-Lim and STFT entry points, said once.  A site names the rules it holds in `rules` and the
// name its messages begin with in `who` ("griffin_lim: ", "stft: ", "" for the general kernels' tables); the answer is the refusal
// text -- empty for a legal call -- and whether it is TTS_ERR_UNSUPPORTED (else TTS_ERR_INVALID).  Where several rules are broken the
// first in this order answers: n_fft, window / hop / T, the lengths of a ragged batch utterance by utterance, the signal's length.
enum : unsigned {
    GL_RULE_NFFT = 1,       // n_fft a power of two, 256 .. 4096 (glg_supports)
    GL_RULE_WINDOW = 2,     // 2 <= window <= n_fft, hop >= 1
    GL_RULE_FRAMES = 4,     // T >= 1
    GL_RULE_SIGNAL = 8,     // hop (T - 1) samples reach beyond the reflect padding
    GL_RULE_ANALYSIS = 16   // the STFT side: T is the signal's samples, and the hop is called "hop"
};
struct GlRefusal { std::string text; bool unsupported = false; };
// lens: the B frame counts of a ragged batch (T is then T_max), each held to 1 .. T_max and to the signal rule; null: none
inline GlRefusal gl_refusal(const std::string& who, unsigned rules, int n_fft, int win, int hop, int T, const int* lens = nullptr, int B = 0) {
    const auto too_short = [&](long long samples) { return samples <= n_fft / 2; };
    const char* const short_text = "signal shorter than n_fft/2 (reflect padding undefined)";
    if ((rules & GL_RULE_NFFT) && (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0))
        return {who + "n_fft must be a power of two between 256 and 4096", true};
    if (((rules & GL_RULE_WINDOW) && (win < 2 || win > n_fft || hop < 1)) || ((rules & GL_RULE_FRAMES) && T < 1)) {
        if (!(rules & GL_RULE_WINDOW)) return {who + "T >= 1"};
        return {who + "need 2 <= win_length <= n_fft, " + ((rules & GL_RULE_ANALYSIS) ? "hop" : "hop_length") + " >= 1" +
                ((rules & GL_RULE_FRAMES) ? ", T >= 1" : "")};
    }
    for (int b = 0; lens && b < B; ++b) {
        if (lens[b] < 1 || lens[b] > T)
            return {who + "n_frames[" + std::to_string(b) + "] = " + std::to_string(lens[b]) + " is not in 1 .. T_max = " + std::to_string(T)};
        if (too_short((long long)hop * (lens[b] - 1)))
            return {who + "utterance " + std::to_string(b) + " (" + std::to_string(lens[b]) + " frames): " + short_text};
    }
    if ((rules & GL_RULE_SIGNAL) && too_short((rules & GL_RULE_ANALYSIS) ? (long long)T : (long long)hop * (T - 1))) return {who + short_text};
    return {};
}

}  // namespace tts
