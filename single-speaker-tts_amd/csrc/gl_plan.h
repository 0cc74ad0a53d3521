// Host side of the streaming Griffin-Lim kernel (gl_stream_kernel, griffin_lim.hip): the constants the kernel and its planner
// share, the ring geometry, the cut of a batch into runs and the per-lane window images.  Plain C++17 -- no HIP type, no
// runtime call -- so that the planner can be compiled and checked without the library (tests/gl_plan_check.cpp).
#pragma once
#include <cstddef>
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

}  // namespace tts
