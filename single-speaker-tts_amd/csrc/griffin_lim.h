// Griffin-Lim / audio kernel launchers shared between griffin_lim.hip and the api_*.hip files.
#pragma once
#include "tts_common.h"
#include "gl_plan.h"

namespace tts {

#define TTS_GL_FP 1056      // padded row length of the frame-major spectra (F = 1025): rows start on 128-byte lines
#define TTS_GL_NFFT tts::NFFT   // the streaming kernel's n_fft (gl_plan.h); every other power of two takes the general path

struct GlParams {
    const float* mag;        // [B][T][FP]
    const float2* phase_in;  // [B][T][FP] 32-bit phasor codes of the current estimate (the pointer type is historical)
    float2* phase_out;       // [B][T][FP]       (iteration)
    float* wav;              // [B][hop*(T-1)]   (final iSTFT)
    float* mse_partial;      // [B][slots_per_utt] or null ([B][T], one per frame, where mom_c is set)
    float* peak_partial;     // [B][slots_per_utt] or null (final iSTFT: per-run max |wav|)
    const float* window;     // [win] periodic hann
    const float* wlane;      // [2][64 lanes][16][2] per-lane window images (gl_build_wlane): analysis / interior synthesis
    const float* rwss;       // [n_fft + hop*(T-1)] 1 / window sum-square (librosa window_sumsquare) where it is > tiny, else 1
    const float2* tw1024;    // exp(-2 pi i k / 1024), k < 1024
    const float2* tw2048;    // exp(-2 pi i k / 2048), k < 1024
    const float2* tables;    // [tw2048 (1024) | W1024^{lane*k2} as [k2-1][lane] (15*64)]: per-lane twiddles, coalesced
    int T, FP, win, hop;
    int B;                   // utterances
    int ncol;                // ceil(win / hop): frames that overlap a sample, halo = ncol - 1
    // work items of a launch: the table of gl_plan_items in device memory (a GlItem is read as an int4); item ids are drawn in
    // table order (first every workgroup's first run, then the runs that follow them)
    const int4* items;
    int n_items, slots_per_utt;
    int n_workers;           // workgroups the cut was made for (= the launch's grid)
    int ring_frames;         // streaming form (gl_stream_kernel): frames an LDS ring holds
    int n_stage;             // ... iterations per launch (1..3), set by launch_gl_stream
    // seeded start (no initial-phase array): the first launch of a call makes the initial phasor of every bin itself
    // (gl_seed_phasor of the seed and the bin's index in the reference's (B, F, T) layout) instead of reading codes
    int seeded, F;
    unsigned long long seed;
    unsigned* work_counter;  // zeroed counter of THIS launch: the persistent workgroups draw item ids from it
    unsigned* clear_counter; // null, or the counter of an EARLIER launch on this stream: one thread zeroes it for a later launch
    // fast Griffin-Lim (momentum, gl_stream_kernel MOM): the projection c of the previous iteration, [B][T][FP] complex, in the
    // kernel's scale (X / 1024), read and rewritten in place by the run that owns a frame; null = the plain iteration.
    // mom_first: the first iteration of a call (t = c: nothing is read, the buffer need not be initialised)
    float2* mom_c;
    float mom_alpha;
    int mom_first;
    // ragged batch (gl_stream_kernel RAG): frames of every utterance, [B] in device memory; T above is then T_max, the stride
    // of every buffer (mag, codes, mom_c, the seeded index, wav rows of hop (T_max - 1)).  rw_edge [B][2][rw_E]: 1 / window
    // sum-square of utterance b's OWN length where it is not the interior image -- its first rw_E entries and its last rw_E
    // (gl_rwss_edges).  Null = one length, T, for all.
    const int* n_frames;
    const float* rw_edge;
    int rw_E;
};

static_assert(sizeof(GlItem) == sizeof(int4), "the kernel reads a GlItem as an int4");

bool gl_stream_instantiated(int win, int hop);                  // the (window, hop) pairs gl_stream_kernel is compiled for (n_fft 2048)
// streaming form of the iteration / final iSTFT (gl_stream_kernel): no chunks, a run is one stream through an LDS ring.
// p needs T, B, win, hop, ncol and the table of a cut (items, n_items, slots_per_utt, n_workers)
hipError_t launch_gl_stream(hipStream_t s, const GlParams& p, int n_cus, int final_istft, int n_stage = 1);
hipError_t gl_configure();
size_t gl_state_bytes();   // bytes per bin of the state between launches (4: a phasor code)
hipError_t launch_gl_mse_reduce(hipStream_t s, const float* partial, int B, int nchunks, float denom, float* mse);
// ragged: mse[b] = sum / (F n_frames[b]); per_frame: the partials are one per frame (the first n_frames[b] of a row of nchunks are summed)
hipError_t launch_gl_mse_reduce_ragged(hipStream_t s, const float* partial, int B, int nchunks, int F, const int* n_frames, int per_frame,
                                       float* mse);
// n_frames (device, [B]) != null in the two launchers that take it: a ragged batch -- columns t >= n_frames[b] are not touched
hipError_t launch_mag_ft_to_tf(hipStream_t s, const float* in, float* out, int B, int F, int T, int FP, const int* n_frames = nullptr);
hipError_t launch_tf_to_ft(hipStream_t s, const float* in, float* out, int B, int F, int T, int FP);
hipError_t launch_phase_init(hipStream_t s, const float* init_ft, uint64_t seed, void* out, int B, int F, int T, int FP, const int* n_frames = nullptr);
hipError_t launch_denorm_power(hipStream_t s, const float* lin, float* mag, size_t rows, int F, int FP,
                               float ref_db, float max_db, float power, int* below_flag);
hipError_t launch_peak_normalize(hipStream_t s, float* wav, int B, int n);
hipError_t launch_peak_scale(hipStream_t s, float* wav, int B, int n, const float* partial, int nparts);
hipError_t launch_stft(hipStream_t s, const float* wav, int B, int n, int Tf, const float* window, int win, int hop,
                       const float2* tw1024, const float2* tw2048, float2* out, int FP);
hipError_t launch_cplx_tf_to_ft(hipStream_t s, const float2* in, float* out, int B, int F, int T, int FP, int mode,
                                float power);
hipError_t launch_db_convert(hipStream_t s, const float* in, float* out, size_t n, int mode, float ref_db, float max_db);
hipError_t launch_any_below(hipStream_t s, const float* in, size_t n, float lim, int* flag);

// general power-of-two path (griffin_lim_generic.hip): one workgroup per frame, FFT in LDS; spectra [B][T][Fp], state =
// float2 unit phasors; tw = exp(-2 pi i k / n_fft), k < n_fft / 2
bool glg_supports(int n_fft);   // power of two, 256 .. 4096
hipError_t glg_configure();
hipError_t launch_glg_phase_init(hipStream_t s, const float* init_ft, uint64_t seed, float2* out, int B, int F, int T, int Fp, const int* n_frames = nullptr);
// frames [B][T][win] scratch; wav [B][hop (T - 1)]: inverse transform of every frame, then the overlap-add (a gather in frame order)
// n_frames != null (device, [B]): a ragged batch -- T is T_max (the stride of every buffer), the workgroups of frames t >= n_frames[b]
// exit, utterance b's signal has hop (n_frames[b] - 1) samples and rwss is [B][n_fft + hop (T - 1)], a row per utterance's own length
hipError_t launch_glg_istft(hipStream_t s, const float* mag, const float2* ph, const float* window, const float* rwss, const float2* tw,
                            float* frames, float* wav, int B, int T, int Fp, int n_fft, int win, int hop, const int* n_frames = nullptr);
// mode 0: out = unit phasors of the spectrum (+ per-frame squared magnitude error against mag when mse_partial != null);
// mode 1: out = the complex spectrum
// mom_c != null (mode 0): the momentum form -- the phasors are those of t = c + alpha (c - previous c), the spectrum c is read
// from and rewritten to mom_c [B][Tf][Fp] (mom_first: t = c, nothing read)
hipError_t launch_glg_stft(hipStream_t s, const float* wav, int n, const float* window, const float2* tw, float2* out, int B, int Tf, int Fp,
                           int n_fft, int win, int hop, int mode, const float* mag, float* mse_partial, float2* mom_c = nullptr,
                           float mom_alpha = 0.f, int mom_first = 0, const int* n_frames = nullptr);

}  // namespace tts
