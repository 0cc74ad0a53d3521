// C ABI, part 3: the call pipeline -- tts_synthesize (three calls in flight on the main, front and encoder streams, events per
// call parity, the wide Griffin-Lim launches), its host-memory form and the tickets of tts_wait_host.
#include "api_internal.h"
#include "encode_plan.h"
#include "token_times_plan.h"

namespace tts_api {

// The launch index from which a pipelined call's Griffin-Lim launches are cut for ALL compute units (gl_run, wide_from), or -1.
// Under the pipeline the next call's decoder starts with this call's first Griffin-Lim launch (its encoder ran in the gap
// before it) on the `reserve_cus` units that Griffin-Lim leaves free, and with the weight-stationary kernel it is done long
// before the last launch (8.9 ms of 12.0 at 64 utterances x 1000 frames): the launches after that would leave 32 units idle.
// Nothing orders the two streams here -- a 256-workgroup launch that finds units still taken runs as 224 workers and its
// last 32 items wait, which costs time (a launch of 0.5 ms becomes 1.0) and never bits -- so the index comes from a model of
// the two durations with half a launch of margin (measured at 64 x 1000 x 60 iterations, GRUCell form, profiles/r05_experiment_gl_wide.txt:
// never 14.74 ms per step, from launch 14: 14.79, 15: 14.49, 16: 14.48, 17: 14.52, 18: 14.56): decoder 0.045 ms per step (both GRU forms; measured 8.9 ms / 200
// steps beside Griffin-Lim), Griffin-Lim 3.1 ns per frame-iteration on the reduced unit count (0.60 ms per launch of
// 3 x 64 x 1000).  A function of the call's shape and the handle's options alone: the waveform's bits do not depend on timing.
int gl_wide_from(tts_handle_t h, const SynthSettings& set, int B, int Ts, int n_steps, int T, int n_iter) {
    if (h->gl_wide == -2 || h->reserve_cus <= 0) return -1;
    const int pd = pd_choice(h, B, Ts, h->reserve_cus, true);
    if (pd == 0) return -1;                    // launch-per-layer decoder: sleeper workgroups hold the units through the whole phase
    if (h->gl_wide >= 0) return h->gl_wide;    // (tools: an explicit launch index)
    if (pd != 2) return -1;                    // the streamed-weights decoder outlasts Griffin-Lim
    const int per_launch = set.gl_momentum > 0 ? 1 : (h->gl_pair < 1 ? 1 : (h->gl_pair > 3 ? 3 : h->gl_pair));   // (as gl_run)
    // The constants were measured on 256 compute units with 32 reserved (224 for Griffin-Lim) at T_s = 150: a launch scales
    // with the units Griffin-Lim really has, a decoder step with the memory length through its attention phase (8.9 of 44.5 us
    // at T_s = 150: keys and values of the whole memory per step, decoder_ws.hip).  On a device of another size the model is
    // not trusted at all: no wide launches there (they only ever cost time, never bits, but a wrong guess costs 0.5 ms a launch).
    if (h->n_cus_dev != 256 || h->n_cus_dev - h->reserve_cus < 16) return -1;
    const double launch_ms = 3.125e-6 * (double)B * T * per_launch * 224.0 / (double)(h->n_cus_dev - h->reserve_cus);
    const double step_ms = (0.0356 + 0.0089 * (double)Ts / 150.0) * (h->cfg.force_cudnn ? 0.038 / 0.045 : 1.0);   // (seven hand-offs per step instead of ten)
    const double dec_ms = step_ms * n_steps + 0.1;
    const int n_launches = (n_iter + per_launch - 1) / per_launch;
    const int from = (int)std::ceil((dec_ms + 0.5 * launch_ms + 0.1) / launch_ms);
    return from <= n_launches ? from : -1;
}

// One tts_synthesize call: its arguments and what the steps below -- in the order they run -- derive from them.
struct SynthCall {
    const int32_t* ids;
    int B, Ts;
    const tts_synth_params_t* sp;
    const float* init_phase;     // the caller's, or null; synth_main puts the estimate here under the option "gl_init"
    float* wav;
    float* mel_out;
    float* align_out;
    float* linear_out;
    const StageArgs* host;       // the upload and encoder signal of tts_synthesize_host (default-constructed otherwise)
    int T, F, FP;
    // the model's window / hop run in the streaming kernel; any other pair in the general kernels (same results to rounding)
    bool gl_streaming;
    float* memory = nullptr;
    float* keys_ahead = nullptr;
    float* mel = nullptr;
    float* magi = nullptr;
    float2* phase_pair[2] = {nullptr, nullptr};
    int parity = 0;
    bool enc_ahead_cfg = false;
    bool pipelined = false;
    int* hold_flag = nullptr;    // synth_order_front: the sleepers' flag, where sleepers hold compute units for this call
    std::optional<GemmGroup> proj;   // synth_front: the decoder's output projection, left to the main stream
    // the handle's settings as they stood when the call was made: nothing of the call reads the handle's own
    SynthSettings set;
    float eos_thr = 0.f;           // end-of-speech stopping: set.eos.threshold_db in the units of `magi`
    int32_t* d_frames = nullptr;   // the lengths on the device (workspace "eos.frames")
    // what the speaking rate and the pitch make of the call's frames
    SynthShape shape;
    int N = 0;                     // the samples of a row of `wav`, hop (Tw - 1): row_samples of that shape
    float* mags = nullptr;         // the time-stretch of `magi`, shape.Tg rows: what Griffin-Lim reconstructs from
    float* gl_wav = nullptr;       // a shifted call: Griffin-Lim's hop (Tg - 1) samples, which the resampler takes into `wav`
    // attention diagnostics: the sentence lengths are taken from the ids behind the encoder, the statistics from `align_out` --
    // the caller's buffer or the handle's -- right behind the decoder, on the decoder's stream
    int32_t* ali_n_sent = nullptr;             // this call parity's lengths on the device (workspace "syn.ali_nsent")
    tts_alignment_stats_t* ali_stats = nullptr;   // where the records go: the host form's buffer set, or workspace "syn.ali_stats"
    // timing marks: the search runs behind the statistics, on the same alignments and lengths
    int32_t* tt_start = nullptr;                   // where its results go: the host form's buffer set, or the stage's scratch
    tts_token_times_stats_t* tt_stats = nullptr;
};

// h->stream is "the stream I enqueue on" for every stage and for ProfScope: the front side of a pipelined call aims it at
// the encoder or front stream, and it is the main stream again on EVERY way out of the scope.
struct StreamScope {
    tts_handle_t h;
    const hipStream_t main_stream;
    explicit StreamScope(tts_handle_t h_) : h(h_), main_stream(h_->stream) {}
    void aim(hipStream_t s) { h->stream = s; }
    ~StreamScope() { h->stream = main_stream; }
};

static long long row_samples(const tts_synth_params_t* sp, const SynthShape& s) { return (long long)sp->hop_length * (s.Tw - 1); }

// The finishing chain, in the order it runs: each stage takes the call's rows in place behind whatever made them (Griffin-Lim, the
// pitch's resampler, the peak normalisation), every utterance over the samples its row holds -- `held`, hop (n[b] - 1) of the reported
// lengths with end-of-speech stopping; null: all N.  Rows no stage can take are refused in the loudness target's name, else the first stage's.
struct FinishStage {
    const char* noun;   // "synthesize: NOUN needs rows of ..."
    bool (*on)(const SynthSettings& set);
    int (*reserve)(tts_handle_t h, int B, int N, const SynthSettings& set);   // (through the stage's own scratch function)
    int (*run)(tts_handle_t h, float* wav, int B, int N, const int32_t* held, const SynthSettings& set);
};
static const FinishStage FINISH[] = {
    {"the equaliser", [](auto& set) { return set.eq.enabled; },   // behind the peak normalisation, ahead of the loudness gain and the limiter
     [](auto h, int B, int N, auto& set) { EqScratch s; return equalizer_scratch(h, B, N, set.eq.n_sections, &s); },
     [](auto h, float* wav, int B, int N, auto held, auto& set) { return equalizer_impl(h, wav, wav, B, N, held, set.eq.sos, set.eq.n_sections); }},
    {"the compressor", [](auto& set) { return set.cmp.enabled; },   // behind the equaliser, ahead of the loudness gain and the limiter
     [](auto h, int B, int N, auto&) { CmpScratch s; return compressor_scratch(h, B, N, false, &s); },
     [](auto h, float* wav, int B, int N, auto held, auto& set) { return compressor_impl(h, wav, wav, B, N, held, set.cmp.params, nullptr, nullptr); }},
    {"the watermark", [](auto& set) { return set.wm.enabled; },   // behind the compressor, ahead of the loudness gain and the limiter: they scale it with the speech
     [](auto h, int B, int N, auto&) { WmScratch s; return watermark_scratch(h, B, N, false, &s); },
     [](auto h, float* wav, int B, int N, auto held, auto& set) { return watermark_impl(h, wav, wav, B, N, held, set.wm.params, nullptr); }},
    {"a loudness target", [](auto& set) { return set.loud.enabled; },   // (with one, nothing ahead of the chain is peak-normalised)
     [](auto h, int B, int N, auto& set) { LoudScratch s; return loudness_scratch(h, B, N, set.loud.sampling_rate, &s); },
     [](auto h, float* wav, int B, int N, auto held, auto& set) {
         return loudness_impl(h, wav, B, N, held, set.loud.sampling_rate, true, set.loud.target_lufs, set.loud.max_peak, nullptr, nullptr, nullptr); }},
    {"the limiter", [](auto& set) { return set.lim.enabled; },   // last: behind the loudness gain, or behind the peak normalisation
     [](auto h, int B, int N, auto&) { LimScratch s; return limiter_scratch(h, B, N, &s); },
     [](auto h, float* wav, int B, int N, auto held, auto& set) { return limiter_impl(h, wav, B, N, held, set.lim.ceiling, set.lim.lookahead, set.lim.oversample, nullptr); }},
};
static const FinishStage* const FINISH_REFUSAL_ORDER[] = {&FINISH[3], &FINISH[0], &FINISH[1], &FINISH[2], &FINISH[4]};

// Step 1: every workspace of the call, sized before anything of it is enqueued (a growing workspace synchronises every stream).
// A stage's buffers come from the stage's own `*_scratch` function (api_internal.h), which the stage asks again for the same
// shape: no name or size of another stage stands here.  The call's own -- the per-parity "syn.*", the stretched magnitudes, the
// shifted call's waveforms, the pinned end-of-speech words -- do.
static int synth_workspaces(tts_handle_t h, SynthCall& k) {
    const tts_config_t& c = h->cfg;
    auto& pl = h->pl;
    const tts_synth_params_t* sp = k.sp;
    const int B = k.B, Ts = k.Ts, T = k.T, FP = k.FP;
    const int Tg = k.shape.Tg;   // (everything of Griffin-Lim is sized for the frames it reconstructs from)
    // A buffer of this call's settings -- momentum, speaking rate, pitch, end-of-speech stopping -- is new or grew: counted in
    // the allocations ws_get makes (h->ws_allocs) across those blocks alone.  The setting was switched on, or to another
    // value, between two calls of a shape, and this call is unpipelined like the first of a shape.  (Not across the other
    // workspaces: a call whose caller stops passing mel_out allocates "syn.mel0" and stays pipelined.)
    bool setting_grew = false;
    unsigned allocs = 0;
    int rc = TTS_OK;
    // Griffin-Lim's workspaces, from the function its kernel family asks again (the two of gl_run); of these only the momentum
    // buffer is a setting's.  (ONE momentum buffer: only Griffin-Lim launches touch it, and those of consecutive calls follow each
    // other on the main stream.  The streaming kernel's partials have room for any cut the call may plan, narrow or wide.)
    GlgScratch gg{};
    GlScratch gs{};
    if (!k.gl_streaming) {   // (and the general kernels' tables)
        const float2* tw_unused = nullptr;
        if ((rc = gl_refuse(h, gl_refusal("griffin_lim: ", GL_RULE_SIGNAL, c.n_fft, sp->win_length, sp->hop_length, Tg))) ||
            (rc = glg_prepare(h, Tg, sp->win_length, sp->hop_length, c.n_fft)) || (rc = glg_twiddles(h, c.n_fft, &tw_unused)) ||
            (rc = glg_scratch(h, B, Tg, sp->win_length, c.n_fft, k.set.gl_momentum, sp->n_iter, &gg)))
            return rc;
    } else if ((rc = gl_scratch(h, B, Tg, k.set.gl_momentum, sp->n_iter, false, 0, false, &gs))) {
        return rc;
    }
    setting_grew |= gg.mom_grew || gs.mom_grew;
    // (one encoder output per call parity: the encoder of call k + 1 writes one while the decoder of call k reads the other)
    WS(h, "syn.memory.even", float, (size_t)B * Ts * 2 * c.n_gru_units, memory_e);
    WS(h, "syn.memory.odd", float, (size_t)B * Ts * 2 * c.n_gru_units, memory_o);
    // (alternating only where the encoder really runs ahead: under the call pipeline with the persistent decoder.  The
    //  launch-per-layer decoder replays a hipGraph with its buffers baked in -- a second `memory` would re-capture it every call)
    k.enc_ahead_cfg = h->enc_stream && h->pipeline && (h->own_stream || h->pipeline >= 2) &&
                      pl.syn_prev.same_network(B, Ts, sp->n_steps) && h->reserve_cus > 0 && pd_choice(h, B, Ts, h->reserve_cus, true) != 0;
    k.memory = (k.enc_ahead_cfg && (pl.syn_calls & 1)) ? memory_o : memory_e;   // (syn_calls is advanced below: this call's parity)
    // the attention keys of that memory, likewise: made behind the encoder on ITS stream, so that nothing but two fills
    // stands between two decoders on the front stream (the 0.04 ms GEMM was on the step's critical path there)
    WS(h, "syn.keys.even", float, (size_t)B * Ts * c.n_attention_units, keys_e);
    WS(h, "syn.keys.odd", float, (size_t)B * Ts * c.n_attention_units, keys_o);
    k.keys_ahead = k.enc_ahead_cfg ? ((pl.syn_calls & 1) ? keys_o : keys_e) : nullptr;
    // The decoder output is double-buffered by call parity: the encoder / decoder of call j+1 (second
    // stream) may then run while the post-net of call j still reads its mel spectrogram.
    const int parity = k.parity = (int)(pl.syn_calls++ & 1);
    k.mel = k.mel_out;
    if (!k.mel) {
        WS(h, "syn.mel0", float, (size_t)B * T * c.n_mels, melb0);
        WS(h, "syn.mel1", float, (size_t)B * T * c.n_mels, melb1);
        k.mel = parity ? melb1 : melb0;
    }
    if ((rc = gl_mag_scratch(h, B, T, FP, &k.magi))) return rc;
    allocs = h->ws_allocs;
    if (k.shape.stretch) {   // (same_call below also compares Tg, which sizes the phasor codes)
        WS(h, "gl.mag_st", float, (size_t)B * Tg * FP, mags);
        k.mags = mags;
    }
    if (k.shape.pitch) {
        WS(h, "gl.wav_pitch", float, (size_t)B * sp->hop_length * (size_t)(Tg - 1), glw);
        k.gl_wav = glw;
    }
    for (const FinishStage& st : FINISH)   // (the finishing chain takes rows of k.N samples)
        if (st.on(k.set) && (rc = st.reserve(h, B, k.N, k.set))) return rc;
    if (k.set.ali.enabled || k.set.tt.enabled) {
        // One alignment buffer and one set of scratch: the statistics of a call run behind its decoder on the decoder's stream,
        // in front of whatever lets the next decoder start.  The sentence lengths are written behind the ENCODER, which may run a
        // call ahead on its own stream: one set per call parity, like `memory`.
        if (!k.align_out) {
            WS(h, "syn.ali", float, (size_t)sp->n_steps * B * Ts, ali_buf);
            k.align_out = ali_buf;
        }
        WS(h, "syn.ali_nsent", int32_t, 2 * (size_t)B, ali_ns);
        k.ali_n_sent = ali_ns + (size_t)parity * B;
        AlignScratch ali;   // (the search takes the positions from it, whoever leaves them there)
        if ((rc = alignment_scratch(h, true, B, sp->n_steps, Ts, &ali))) return rc;
    }
    if (k.set.tt.enabled) {
        TokenTimesScratch tt;
        if ((rc = token_times_scratch(h, true, B, sp->n_steps, Ts, &tt))) return rc;
        k.tt_start = k.host->tt_start_out ? k.host->tt_start_out : tt.start;
        k.tt_stats = k.host->tt_stats_out ? k.host->tt_stats_out : tt.stats;
    }
    if (k.set.ali.enabled) {
        k.ali_stats = k.host->stats_out;
        if (!k.ali_stats) {
            WS(h, "syn.ali_stats", tts_alignment_stats_t, (size_t)B, ali_st);
            k.ali_stats = ali_st;
        }
    }
    // (estimated initial phases, option "gl_init": the estimate's buffers, for the frames Griffin-Lim reconstructs from)
    PhaseScratch est;
    if (k.set.gl_init && !k.init_phase && (rc = phase_estimate_scratch(h, B, Tg, c.n_fft, false, true, &est))) return rc;
    setting_grew |= h->ws_allocs != allocs;
    // Under the call pipeline the initial phasors of a call are written on the FRONT stream, behind its decoder (that
    // stream has slack, the main one bounds the step): the phasor-code buffers are then a pair per call parity, so that
    // the write does not wait for the previous call's Griffin-Lim.  All four are sized here, before anything is enqueued
    // (a growing workspace synchronises every stream).
    // (its own buffers, not the pair of the stand-alone tts_griffin_lim: 4 bytes per bin, the state is a phasor code)
    WS(h, "syn.phase0.even", unsigned, (size_t)B * Tg * FP * (gl_state_bytes() / sizeof(unsigned)), gph0e);
    WS(h, "syn.phase1.even", unsigned, (size_t)B * Tg * FP * (gl_state_bytes() / sizeof(unsigned)), gph1e);
    WS(h, "syn.phase0.odd", unsigned, (size_t)B * Tg * FP * (gl_state_bytes() / sizeof(unsigned)), gph0o);
    WS(h, "syn.phase1.odd", unsigned, (size_t)B * Tg * FP * (gl_state_bytes() / sizeof(unsigned)), gph1o);
    allocs = h->ws_allocs;
    if (k.set.eos.enabled) {
        // the detection's row flags and lengths (speech_frames_impl asks eos_scratch again), the ragged Griffin-Lim's tables
        // (gl_rag_tables asks gl_rag_scratch again; with a speaking rate the stretched lengths are the host's, which it uploads)
        // and the pinned words the host reads the lengths from: nothing grows in mid-call
        // (a larger stand-alone ragged call may have left smaller buffers: growing them counts like making them)
        EosScratch eos;
        RagScratch rag;
        if ((rc = eos_scratch(h, B, T, true, &eos)) ||
            (rc = gl_rag_scratch(h, B, Tg, sp->win_length, sp->hop_length, c.n_fft, k.gl_streaming, k.shape.stretch, &rag)))
            return rc;
        k.d_frames = eos.frames;
        if (h->eos.pinned_room < B) {   // (read behind a synchronisation inside the call that filled it: never in flight here)
            setting_grew = true;
            if (h->eos.pinned) HIPCHK(h, hipHostFree(h->eos.pinned));
            h->eos.pinned = nullptr;
            h->eos.pinned_room = 0;
            HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&h->eos.pinned), (size_t)B * sizeof(int32_t), hipHostMallocDefault));
            h->eos.pinned_room = B;
        }
    }
    setting_grew |= h->ws_allocs != allocs;
    k.phase_pair[0] = reinterpret_cast<float2*>(parity ? gph0o : gph0e);
    k.phase_pair[1] = reinterpret_cast<float2*>(parity ? gph1o : gph1e);
    // Pipelined only while the library owns its stream (inputs on a borrowed stream may still be in flight) and
    // from the second call of a shape on: the first call of a new (B, Ts, n_steps) grows the workspaces, which
    // synchronises every stream -- under the CU reservation that would park the host on the sleepers' 100 ms bound.
    // (a setting switched between two calls of a shape: another Tg or another pitch in the key, or a buffer of the setting
    //  that is new -- setting_grew above)
    const CallPipeline::SynKey key{B, Ts, sp->n_steps, Tg, k.shape.pitch ? k.shape.rho : 0.0};
    const bool same_call = key == pl.syn_prev && !setting_grew;
    pl.syn_prev = key;
    // (a borrowed stream is pipelined only on request, pipeline = 2: the caller then vouches that the inputs of a call
    //  are complete when it is made -- the library cannot tell them from the previous call's work on that stream)
    k.pipelined = h->pipeline && (h->own_stream || h->pipeline >= 2) && same_call;
    return TTS_OK;
}

// Step 2, the first pipelined call of a handle: the front, sleeper and encoder streams and the sleepers' flags.
static int synth_streams(tts_handle_t h) {
    auto& pl = h->pl;
    if (pl.front) return TTS_OK;
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIPCHK(h, hipStreamCreateWithPriority(&pl.front, hipStreamNonBlocking, prio_greatest));
    HIPCHK(h, hipStreamCreateWithPriority(&pl.aux, hipStreamNonBlocking, prio_greatest));
    // (lowest priority: at the front stream's priority the encoder takes more from the post-net beside it than the
    //  decoder's head start is worth -- 17.11 against 16.87 ms per step on one box; a third queue costs the
    //  Griffin-Lim launches 3-4 % whatever its priority, which is why the step is not the decoder's 15.6 ms)
    HIPCHK(h, hipStreamCreateWithPriority(&pl.encs, hipStreamNonBlocking, prio_least));
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&pl.hold_flags), 2 * sizeof(int)));
    HIPCHK(h, cu_hold_configure());
    // calls made before these streams existed recorded nothing: the front stream's first work starts behind
    // everything that is on the main stream now
    HIPCHK(h, pl.aux_mark.record(h->stream));
    HIPCHK(h, pl.aux_mark.wait(pl.front));
    HIPCHK(h, pl.aux_mark.wait(pl.encs));
    return TTS_OK;
}

// Step 3: the waits in front of this call's encoder and decoder, on the streams they will run on (*enc_on: the encoder's).
static int synth_order_front(tts_handle_t h, SynthCall& k, hipStream_t* enc_on) {
    auto& pl = h->pl;
    const int B = k.B, Ts = k.Ts, parity = k.parity;
    *enc_on = h->stream;
    if (k.pipelined) {
        // The persistent decoder keeps its compute units by being resident (Griffin-Lim is planned and launched for
        // the other n_cus - reserve_cus), and the encoder in front of it may queue behind Griffin-Lim workgroups
        // without costing the step anything: no sleepers then.  The launch-per-layer decoder (configurations the
        // persistent kernel does not cover) still needs the reservation for its ~2000 dependent launches.
        const bool pd_path = h->reserve_cus > 0 && pd_choice(h, B, Ts, h->reserve_cus, true) != 0;
        // the post-net of the call two back read the mel buffer this call's decoder writes; with a caller's
        // mel buffer (possibly the same one every call) the previous call's post-net has to finish as well
        HIPCHK(h, pl.post_done[parity].wait(pl.front));
        // an unpipelined call in between ran its encoder and decoder on the MAIN stream, in the scratch buffers this
        // call's encoder and decoder are about to use on the front stream
        HIPCHK(h, pl.serial_done.wait(pl.front));
        HIPCHK(h, pl.serial_done.wait(pl.encs));
        pl.serial_done.disarm();
        if (k.mel_out) HIPCHK(h, pl.post_done[parity ^ 1].wait(pl.front));
        // The call two back ends its Griffin-Lim phase in launches cut for ALL compute units (gl_wide_from): this call's
        // decoder must not take 32 of them away in the middle of those, so it starts behind the post-net of the call before
        // it, i.e. behind that whole phase.  In the steady state this is where it starts anyway (its encoder runs beside that
        // post-net); it matters while a burst of calls fills the pipeline, when the decoders -- 8.9 ms against 14.5 per call
        // on the main stream -- would run ahead back to back (profiles/r05_step_timeline.txt before the gate: the wide
        // launches of calls 2 and 3 took 0.77 instead of 0.55 ms).  Only then: where the decoder is the longer stage (small
        // batches) there are no wide launches, and this wait would put the post-net into the decoders' chain.
        if (pl.gl_wide_used[parity]) HIPCHK(h, pl.post_done[parity ^ 1].wait(pl.front));
        if (h->reserve_cus > 0 && !pd_path) {
            // reserve CUs for the front stream while the previous call's Griffin-Lim fills the rest
            k.hold_flag = pl.hold_flags + (pl.call_count++ & 1);
            // the persistent decoder releases its call's sleepers as soon as it is resident: the next set must not
            // start (and take another `reserve_cus` away from Griffin-Lim) before that decoder has finished
            HIPCHK(h, pl.front_done.wait(pl.aux));
            HIPCHK(h, hipMemsetAsync(k.hold_flag, 0, sizeof(int), pl.aux));
            HIPCHK(h, pl.aux_mark.record(pl.aux));
            HIPCHK(h, launch_cu_hold(pl.aux, h->reserve_cus, k.hold_flag, 100.0, h->hold_lds_kb));
            HIPCHK(h, pl.aux_mark.wait(pl.front));
            HIPCHK(h, pl.aux_mark.wait(pl.encs));
        }
        // the encoder: on its own stream, behind the decoder that last read this parity's `memory` (the call two back) and
        // behind the encoder before it (stream order: the encoder's scratch is one set)
        if (k.enc_ahead_cfg) {
            HIPCHK(h, pl.dec_done[parity].wait(pl.encs));
            // ... which is enough only if the previous call ran encoder-ahead too.  A call in the other form (the decoder
            // form was switched in between: tts_set_option, or tts_wait_host / check_status after a decoder timeout) ran its
            // encoder AND decoder on `front`, in the one encoder scratch and in memory.even: behind its decoder, the last
            // thing recorded on that stream
            if (pl.last_enc_ahead == 0) HIPCHK(h, pl.dec_done[parity ^ 1].wait(pl.encs));
            // The HOST waits for the gap (the call returns at most ~2.5 calls ahead of the device: back-pressure), and the
            // encoder is enqueued into an idle queue.  As a stream wait, enqueued two calls early, the barrier packet sat at
            // the head of the third queue through a whole Griffin-Lim phase, and every kernel boundary of that phase took
            // ~18 us longer (13.16 against 12.67 ms per call on one box, whatever the queue's priority).
            HIPCHK(h, pl.gap[parity].sync());
            *enc_on = pl.encs;
        } else {
            // the encoder in front of its decoder on the front stream (one `memory` buffer): behind whatever encoders and
            // decoders of earlier calls are still on the encoder / front streams (the front stream's own order covers the latter)
            for (int i = 0; i < 2; ++i) HIPCHK(h, pl.enc_ready[i].wait(pl.front));
            *enc_on = pl.front;
        }
        pl.last_enc_ahead = k.enc_ahead_cfg ? 1 : 0;
    } else if (pl.encs) {
        // an unpipelined call runs its encoder and decoder on the main stream in the same scratch: behind whatever the
        // pipelined calls before it still have on the encoder and front streams
        for (int i = 0; i < 2; ++i) {
            HIPCHK(h, pl.enc_ready[i].wait(h->stream));
            HIPCHK(h, pl.dec_done[i].wait(h->stream));
        }
    }
    return TTS_OK;
}

// Step 4: the ids' upload (host calls), encoder, attention keys and decoder -- on `enc_on` and the front stream of a pipelined
// call, on the main stream otherwise.
static int synth_front(tts_handle_t h, SynthCall& k, hipStream_t enc_on) {
    auto& pl = h->pl;
    const int B = k.B, Ts = k.Ts, parity = k.parity;
    int rc = TTS_OK;
    StreamScope on(h);
    on.aim(enc_on);
    if (k.host->upload.bytes) {   // (tts_synthesize_host: the ids' upload, in front of the encoder on its own stream)
        const auto& up = k.host->upload;
        if (k.host->enc_done) HIPCHK(h, k.host->enc_done->wait(h->stream));
        HIPCHK(h, hipMemcpyAsync(up.dst, up.src, up.bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, up.done->record(h->stream));
    }
    if ((rc = encoder_impl(h, k.ids, B, Ts, k.memory))) return rc;
    // (attention diagnostics: the sentence lengths, where the ids are certainly in place -- beside the encoder that reads them)
    // (... once, for the statistics and the timing marks alike: with both on, the statistics' padding is the one)
    if ((k.set.ali.enabled || k.set.tt.enabled) &&
        (rc = text_lengths_impl(h, k.ids, B, Ts, k.set.ali.enabled ? k.set.ali.pad_id : k.set.tt.pad_id, k.ali_n_sent)))
        return rc;
    if (k.host->enc_done) HIPCHK(h, k.host->enc_done->record(h->stream));
    if (k.pipelined && k.keys_ahead) {
        ProfScope ps(h, ST_ENCODER, 1);
        if ((rc = attention_keys(h, k.memory, B, Ts, k.keys_ahead))) return rc;
    }
    if (k.pipelined) {
        if (k.enc_ahead_cfg) {
            HIPCHK(h, pl.enc_ready[parity].record(pl.encs));
            HIPCHK(h, pl.enc_ready[parity].wait(pl.front));
        }
        on.aim(pl.front);
    }
    StageArgs args;
    args.hold_flag = k.hold_flag;
    args.cu_budget = (k.pipelined && h->reserve_cus > 0) ? h->reserve_cus : 0;
    // nothing in flight on the main stream: no post-net, no Griffin-Lim runs beside this call's decoder (the first call of a
    // burst) -- the weight-stationary decoder may then spread over twice the compute units (decoder_impl; the same bits)
    args.chip_idle = k.pipelined && hipStreamQuery(on.main_stream) == hipSuccess;
    args.project_later = k.pipelined;
    args.parity = parity;
    args.keys = k.pipelined ? k.keys_ahead : nullptr;
    if ((rc = decoder_impl(h, k.memory, B, Ts, k.sp->n_steps, k.mel, k.align_out, nullptr, args, &k.proj))) return rc;
    if (k.set.ali.enabled) {
        // Attention diagnostics: right behind the decoder on its stream and in front of the records below, so that whatever
        // waits for this decoder -- the next one, an encoder that reuses this parity's lengths -- waits for the statistics too
        if ((rc = alignment_impl(h, k.align_out, k.sp->n_steps, B, Ts, nullptr, nullptr, k.ali_n_sent, k.ali_stats, nullptr, nullptr, nullptr)))
            return rc;
        HIPCHK(h, h->ali.done.record(h->stream));
        h->ali.last_dev = k.ali_stats;
        h->ali.last_B = B;
    }
    if (k.set.tt.enabled) {
        // Timing marks: the search, behind the statistics whose positions it reads, in front of the records below like them
        if ((rc = token_times_impl(h, k.align_out, k.sp->n_steps, B, Ts, nullptr, nullptr, k.ali_n_sent, k.set.ali.enabled, k.set.tt.max_jump,
                                   k.tt_start, nullptr, k.tt_stats)))
            return rc;
        HIPCHK(h, h->tt.done.record(h->stream));
        h->tt.last_start = k.tt_start;
        h->tt.last_stats = k.tt_stats;
        h->tt.last_B = B;
        h->tt.last_Ts = Ts;
    }
    if (k.pipelined) HIPCHK(h, pl.dec_done[parity].record(pl.front));
    else if (pl.front) HIPCHK(h, pl.serial_done.record(on.main_stream));
    return TTS_OK;
}

// Step 5a, end-of-speech stopping: the lengths of this call's utterances, from its magnitudes on the main stream to h->eos.pinned.
// The HOST waits here for the post-net.  Everything this call puts on the front and encoder streams has been enqueued by now,
// and the call returns as soon as the lengths are read and its Griffin-Lim is enqueued: the next call's encoder and decoder,
// enqueued by that call, run beside this call's Griffin-Lim as they do without the wait.  What the wait costs (1.0 ms per
// batch at 64 x 1000 frames, profiles/eos.txt) is mostly WHEN the next call gets made: its encoder starts beside the first
// Griffin-Lim launches instead of beside this post-net; the detection is 0.06 ms, the read-back and the enqueue a launch gap.
static int synth_detect(tts_handle_t h, SynthCall& k) {
    const int B = k.B, T = k.T, min_frames = k.shape.min_frames;
    int rc = speech_frames_impl(h, k.magi, B, T, k.F, k.FP, k.eos_thr, k.set.eos.keep_frames, min_frames, k.d_frames, nullptr);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->eos.pinned, k.d_frames, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // (what the launches below are cut for and index with: checked again on this side)
    for (int b = 0; b < B; ++b)
        if (h->eos.pinned[b] < min_frames || h->eos.pinned[b] > T)
            return fail(h, TTS_ERR_HIP, "synthesize: the end-of-speech detection returned " + std::to_string(h->eos.pinned[b]) +
                                            " frames for utterance " + std::to_string(b) + ", outside [" + std::to_string(min_frames) +
                                            ", " + std::to_string(T) + "]");
    return TTS_OK;
}

// Step 5: the main stream takes over behind the front stream -- the decoder's output projection, post-net and Griffin-Lim.
static int synth_main(tts_handle_t h, SynthCall& k) {
    auto& pl = h->pl;
    const tts_synth_params_t* sp = k.sp;
    const SynthShape& s = k.shape;
    const int B = k.B, T = k.T, Tg = s.Tg, parity = k.parity;
    int rc = TTS_OK;
    // (a seeded start with iterations needs no initial codes at all: gl_run.  Estimated phases -- option "gl_init" without an
    //  explicit init_phase -- come from this call's magnitudes, which do not exist yet: they are made on the main stream below)
    const bool estimate = k.set.gl_init && !k.init_phase;
    const bool phase_on_front = !estimate && k.gl_streaming && k.pipelined && sp->n_iter >= 0 && (k.init_phase != nullptr || sp->n_iter == 0);
    if (k.pipelined) {
        if (k.hold_flag) HIPCHK(h, hipMemsetAsync(k.hold_flag, 1, sizeof(int), pl.front));   // release the held CUs
        if (phase_on_front) {
            // this parity's buffers were last used by the Griffin-Lim of the call two back
            HIPCHK(h, pl.gl_done[parity].wait(pl.front));
            HIPCHK(h, launch_phase_init(pl.front, k.init_phase, sp->seed, k.phase_pair[0], B, k.F, Tg, k.FP));
        }
        HIPCHK(h, pl.front_done.record(pl.front));
        HIPCHK(h, pl.front_done.wait(h->stream));
    }
    // the decoder's output projection, on the main stream (see StageArgs::project_later)
    if (k.proj && (rc = run_single(h, *k.proj))) return rc;
    // the gap between two Griffin-Lim phases opens: the encoder of the next call of this parity may run
    if (pl.encs) HIPCHK(h, pl.gap[parity].record(h->stream));
    int* db_flag = nullptr;
    if (denorm_can_assert(sp->ref_db, sp->max_db) && (rc = denorm_flag_arm(h, &db_flag))) return rc;
    // linear_out null: the final Dense emits only the de-normalised magnitude (rows of 1028 floats; the 1025-float rows of the
    // linear spectrogram cannot be written in whole cache lines)
    if ((rc = postnet_impl(h, k.mel, B, T, k.linear_out, k.magi, sp->ref_db, sp->max_db, sp->power, db_flag))) return rc;
    if (db_flag && (rc = denorm_flag_read(h))) return rc;   // as the reference: no waveform for such a spectrogram
    // (also for an unpipelined call between pipelined ones: its buffers are the same ones)
    if (pl.front) HIPCHK(h, pl.post_done[parity].record(h->stream));
    // the lengths (synth_plan.h): all T without end-of-speech stopping -- and a call that stops nowhere IS the uniform call
    const int32_t* detected = nullptr;
    if (k.set.eos.enabled) {
        if ((rc = synth_detect(h, k))) return rc;
        detected = h->eos.pinned;
    }
    SynthLengths& L = h->syn_lens;
    synth_lengths(s, T, sp->hop_length, B, detected, &L);
    h->eos.last = L.reported;
    // The speaking rate: Griffin-Lim reconstructs from the time-stretch of this call's magnitudes (one pass, stretch.hip).
    // Frames behind an utterance's end are not read; whatever the stretched length adds to an utterance is the vocoder's zero
    // padding, which the pass writes.
    if (s.stretch && (rc = stretch_impl(h, k.magi, B, T, k.F, k.FP, true, detected, s.rate, Tg, k.mags))) return rc;
    const int32_t* n_frames = L.ragged ? L.gl.data() : nullptr;
    const float* gl_mag = s.stretch ? k.mags : k.magi;
    // (the device's lengths are those of the detection: with a speaking rate the host's stretched ones are uploaded instead)
    const int* d_frames = (n_frames && !s.stretch) ? k.d_frames : nullptr;
    // estimated initial phases: from the magnitudes Griffin-Lim reconstructs from, at each utterance's own length, between the
    // post-net (or the stretch) and the first Griffin-Lim launch; from here on they are the call's explicit init_phase
    const float* init_phase = k.init_phase;
    if (estimate && (rc = gl_init_phase(h, k.set.gl_init, gl_mag, nullptr, B, Tg, k.FP, n_frames, h->cfg.n_fft, sp->hop_length, &init_phase))) return rc;
    const int wide_from = (k.pipelined && k.gl_streaming) ? gl_wide_from(h, k.set, B, k.Ts, sp->n_steps, L.T_model, sp->n_iter) : -1;
    pl.gl_wide_used[parity] = wide_from >= 0;
    float* gl_wav = s.pitch ? k.gl_wav : k.wav;
    // (a shifted call normalises what the resampler leaves; with a loudness target nothing is peak-normalised)
    const bool gl_peak = sp->peak_normalize != 0 && !s.pitch && !k.set.loud.enabled;
    GlCall gl;
    gl.mag = gl_mag; gl.init_ft = init_phase; gl.seed = sp->seed;
    gl.B = B; gl.T = Tg; gl.n_iter = sp->n_iter; gl.win = sp->win_length; gl.hop = sp->hop_length; gl.n_fft = h->cfg.n_fft;
    gl.wav = gl_wav; gl.peak_normalize = gl_peak; gl.n_frames = n_frames; gl.d_frames = d_frames;
    gl.momentum = k.set.gl_momentum;   // (the call's own copy of the setting, as synth_workspaces and gl_wide_from took it)
    gl.under_reservation = k.pipelined; gl.phase_pair = k.phase_pair; gl.phase_ready = phase_on_front; gl.wide_from = wide_from;
    rc = gl_run(h, gl);   // (the family k.gl_streaming names: gl_is_streaming of the same three numbers)
    if (s.pitch && !rc) {
        // The pitch: the hop (Tg - 1) samples Griffin-Lim made, resampled by rho into the rows of the call without pitch.  With
        // end-of-speech stopping utterance b has hop (n'[b] - 1) samples, and its row ends where the un-shifted call's does.
        const int n_gl = sp->hop_length * (Tg - 1);
        rc = resample_impl(h, k.gl_wav, B, n_gl, detected ? L.n_samples.data() : nullptr, s.rho, k.N, detected ? L.keep.data() : nullptr, k.wav);
        if (!rc && sp->peak_normalize && !k.set.loud.enabled) HIPCHK(h, launch_peak_normalize(h->stream, k.wav, B, k.N));
    }
    // The finishing chain (FINISH), in place, over the samples each row holds
    std::vector<int32_t> held;
    if (detected && std::any_of(std::begin(FINISH), std::end(FINISH), [&](const FinishStage& st) { return st.on(k.set); }))
        for (int b = 0; b < B; ++b) held.push_back(sp->hop_length * (L.reported[(size_t)b] - 1));
    for (const FinishStage& st : FINISH)
        if (!rc && st.on(k.set)) rc = st.run(h, k.wav, B, k.N, detected ? held.data() : nullptr, k.set);
    if (pl.front && !rc) HIPCHK(h, pl.gl_done[parity].record(h->stream));
    return rc;
}

// tts_synthesize on a ready handle; `set`: the copy of the handle's settings the entry point took, `host` carries the upload of
// tts_synthesize_host
static int synthesize_impl(tts_handle_t h, const SynthSettings& set, const int32_t* ids, int B, int Ts, const tts_synth_params_t* sp,
                           const float* init_phase, float* wav, float* mel_out, float* align_out, float* linear_out, const StageArgs& host) {
    int rc = TTS_OK;
    if (!ids || !sp || !wav || B < 1 || Ts < 1 || sp->n_steps < 1) return fail(h, TTS_ERR_INVALID, "synthesize: bad arguments");
    const tts_config_t& c = h->cfg;
    // n_fft is a model parameter (reference tacotron/params/model.py:13-24): the final Dense has 1 + n_fft / 2 outputs, its
    // de-normalising epilogue writes rows padded to gl_fp(n_fft), and every size but 2048 reconstructs in the general kernels
    if ((rc = gl_refuse(h, gl_refusal("synthesize: ", GL_RULE_NFFT, c.n_fft, 0, 0, 0)))) return rc;
    SynthCall k{ids, B, Ts, sp, init_phase, wav, mel_out, align_out, linear_out, &host, sp->n_steps * c.reduction,
                1 + c.n_fft / 2, gl_fp(c.n_fft), gl_is_streaming(c.n_fft, sp->win_length, sp->hop_length)};
    k.set = set;
    // (refusals come before anything is enqueued; rate 1.0 and pitch 0: nothing of this call changes)
    const std::string refusal = synth_shape(k.T, c.n_fft, sp->hop_length, set.speaking_rate, set.pitch_octaves, set.eos.enabled != 0, &k.shape);
    if (!refusal.empty()) return fail(h, TTS_ERR_INVALID, "synthesize: " + refusal);
    const double* tab_unused = nullptr;   // (the ratio's table, made before anything of this call is enqueued)
    if (k.shape.pitch && (rc = resample_table(h, k.shape.rho, &tab_unused))) return rc;
    if (k.gl_streaming && (rc = gl_prepare(h, k.shape.Tg, sp->win_length, sp->hop_length, c.n_fft))) return rc;
    if (!k.gl_streaming && (rc = gl_refuse(h, gl_refusal("synthesize: ", GL_RULE_WINDOW, c.n_fft, sp->win_length, sp->hop_length, 0)))) return rc;
    if (set.eos.enabled && speech_threshold(set.eos.threshold_db, sp->ref_db, sp->max_db, sp->power, TTS_SPEECH_MAGNITUDE_POWER, &k.eos_thr))
        return fail(h, TTS_ERR_INVALID, "synthesize: end-of-speech stopping needs power > 0");
    const long long n_rows = row_samples(sp, k.shape);
    k.N = (int)n_rows;
    for (const FinishStage* st : FINISH_REFUSAL_ORDER)
        if (st->on(set) && (sp->hop_length < 1 || n_rows < 1 || n_rows > INT32_MAX))
            return fail(h, TTS_ERR_INVALID, std::string("synthesize: ") + st->noun + " needs rows of 1 .. 2^31 - 1 samples");
    h->ali.last_dev = nullptr;   // (the records of a call before this one are no longer "the last call's")
    h->tt.last_start = nullptr;
    h->tt.last_stats = nullptr;
    if (set.tt.enabled && Ts > TT_MAX_TOKENS) return fail(h, TTS_ERR_UNSUPPORTED, "synthesize: token times: " + token_times_unsupported(Ts));
    if ((rc = synth_workspaces(h, k))) return rc;
    if (k.pipelined && (rc = synth_streams(h))) return rc;
    hipStream_t enc_on = nullptr;
    if (!(rc = synth_order_front(h, k, &enc_on))) rc = synth_front(h, k, enc_on);
    if (rc) {   // (the sleepers of this call, if they were started, must not hold their compute units for the 100 ms bound)
        if (k.hold_flag) hipMemsetAsync(k.hold_flag, 1, sizeof(int), h->pl.front);
        return rc;
    }
    return synth_main(h, k);
}

}  // namespace tts_api

// ======================================================================================== C ABI
extern "C" {

int tts_synthesize(tts_handle_t h, const int32_t* ids, int B, int Ts, const tts_synth_params_t* sp,
                   const float* init_phase, float* wav, float* mel_out, float* align_out, float* linear_out) {
    DeviceScope dev_scope(h);
    const int rc = check_ready(h);
    if (rc) return rc;
    return synthesize_impl(h, h->settings, ids, B, Ts, sp, init_phase, wav, mel_out, align_out, linear_out, StageArgs());
}

// Host-memory form of tts_synthesize (see sstts_hip.h): uploads and downloads on copy streams, ordered by events, so that
// consecutive calls overlap exactly like calls on device-resident buffers.
int tts_synthesize_host(tts_handle_t h, const int32_t* ids_host, int B, int Ts, const tts_synth_params_t* sp, int* ticket) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!ids_host || !sp || !ticket || B < 1 || Ts < 1 || sp->n_steps < 1)
        return fail(h, TTS_ERR_INVALID, "synthesize_host: bad arguments");
    const SynthSettings set = h->settings;   // (the one copy this call and everything it enqueues is made from)
    auto& io = h->hio;
    const int T = sp->n_steps * h->cfg.reduction;
    // (with a speaking rate the waveforms have hop (Tw - 1) samples: the pinned and device buffers are sized for them.  What
    //  the plan refuses is synthesize_impl's to report, below; Tw = stretched_frames(T, speaking_rate) stands either way)
    SynthShape shape;
    synth_shape(T, h->cfg.n_fft, sp->hop_length, set.speaking_rate, set.pitch_octaves, set.eos.enabled != 0, &shape);
    const size_t ids_bytes = (size_t)B * Ts * sizeof(int32_t);
    const long long N_rows = row_samples(sp, shape);
    const size_t n_wav = (size_t)B * (size_t)N_rows;
    const bool want_lin = (sp->host_outputs & TTS_HOST_LINEAR) != 0, want_ali = (sp->host_outputs & TTS_HOST_ALIGNMENTS) != 0;
    const size_t n_lin = want_lin ? (size_t)B * T * (size_t)(1 + h->cfg.n_fft / 2) : 0;
    const size_t n_ali = want_ali ? (size_t)sp->n_steps * B * Ts : 0;
    const size_t stats_bytes = set.ali.enabled ? (size_t)B * sizeof(tts_alignment_stats_t) : 0;
    const size_t tt_start_bytes = set.tt.enabled ? (size_t)B * (size_t)(Ts + 1) * sizeof(int32_t) : 0;
    const size_t tt_stats_bytes = set.tt.enabled ? (size_t)B * sizeof(tts_token_times_stats_t) : 0;
    // The delivery format (tts_set_output): the float32 rows stay on the device, the resampler takes them -- each over the samples
    // it holds -- into rows of N_enc samples, and the encoder's codes travel instead.  Everything that may allocate -- the staging
    // buffers, the ratio's table, the resampled rows, which are a workspace -- is made here, before anything is enqueued.
    const bool encoded = set.out.enabled, resampled = encoded && set.out.ratio != 1.0, coded = encoded && set.out.format != ENC_F32;
    long long N_enc = N_rows;
    if (encoded && (sp->hop_length < 1 || N_rows < 1 || N_rows > INT32_MAX))
        return fail(h, TTS_ERR_INVALID, "synthesize_host: a delivery format needs rows of 1 .. 2^31 - 1 samples");
    if (resampled && (N_enc = resampled_length((int)N_rows, set.out.ratio)) > INT32_MAX)
        return fail(h, TTS_ERR_INVALID, "synthesize_host: the resampled rows have more than 2^31 - 1 samples");
    const size_t code_bytes = encoded ? (size_t)B * (size_t)N_enc * (size_t)enc_width(set.out.format) : 0;
    const size_t rec_bytes = coded ? (size_t)B * sizeof(tts_encode_stats_t) : 0;
    float* rs_rows = nullptr;
    if (resampled) {
        const double* tab_unused = nullptr;
        if ((rc = resample_table(h, set.out.ratio, &tab_unused))) return rc;
        if (coded) {   // (without an encoding the resampler writes the set's buffer itself)
            WS(h, "out.resampled", float, (size_t)B * (size_t)N_enc, rows);
            rs_rows = rows;
        }
    }
    if (!io.out) {
        // The copy stream gets the LOWEST priority: streams of one priority share a few hardware queues in creation order
        // (whatever else the process has created counts; GPU_MAX_HW_QUEUES per priority, as few as 2), and a copy stream that
        // lands on the main stream's queue holds the main stream's kernels behind its event waits and its 70 MB download.
        // The only other stream at this level is the encoder's; the ids' upload rides on that one (in tts_synthesize), since
        // a second copy stream there would share a queue with it and park the encoder of call k + 2 behind the download of k.
        int prio_least = 0, prio_greatest = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        HIPCHK(h, hipStreamCreateWithPriority(&io.out, hipStreamNonBlocking, prio_least));
        HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&io.status_pinned), 6 * sizeof(int), hipHostMallocDefault));
    }
    // (the sets grow together and the last one last: it fits where all of them do)
    if (ids_bytes > io.ids[2].bytes || n_wav * sizeof(float) > io.wav[2].bytes || n_lin * sizeof(float) > io.lin[2].bytes ||
        n_ali * sizeof(float) > io.ali[2].bytes || stats_bytes > io.stats[2].bytes || code_bytes > io.codes[2].bytes ||
        rec_bytes > io.enc_stats[2].bytes || tt_start_bytes > io.tt_start[2].bytes || tt_stats_bytes > io.tt_stats[2].bytes) {
        // growing the buffers: nothing of an earlier call may be in flight
        if ((rc = sync_all(h))) return rc;
        HIPCHK(h, hipStreamSynchronize(io.out));
        for (int i = 0; i < 3; ++i) {
            HIPCHK(h, io.ids[i].grow(ids_bytes));
            HIPCHK(h, io.wav[i].grow(n_wav * sizeof(float)));
            HIPCHK(h, io.lin[i].grow(n_lin * sizeof(float)));
            HIPCHK(h, io.ali[i].grow(n_ali * sizeof(float)));
            HIPCHK(h, io.stats[i].grow(stats_bytes));
            HIPCHK(h, io.codes[i].grow(code_bytes));
            HIPCHK(h, io.enc_stats[i].grow(rec_bytes));
            HIPCHK(h, io.tt_start[i].grow(tt_start_bytes));
            HIPCHK(h, io.tt_stats[i].grow(tt_stats_bytes));
        }
        io.reset();
    }
    const int t = io.tickets++;
    const int par = t % 3;   // (buffer set of this call; the device-side pipeline keeps its own parity)
    // the pinned staging buffer and the device copy of the ids were last used by the call three back
    HIPCHK(h, io.h2d[par].sync());
    std::memcpy(io.ids[par].pinned, ids_host, ids_bytes);
    // the waveform buffer of this set is free once the download of the call three back has left it
    HIPCHK(h, io.d2h[par].wait(h->stream));
    // the device copy of the ids is free once the encoder of the call three back has read it (the same stream as a rule)
    StageArgs host;
    host.upload.dst = io.ids[par].dev;
    host.upload.src = io.ids[par].pinned;
    host.upload.bytes = ids_bytes;
    host.upload.done = &io.h2d[par];
    host.enc_done = &io.enc[par];
    host.stats_out = stats_bytes ? io.stats[par].dev : nullptr;
    host.tt_start_out = tt_start_bytes ? io.tt_start[par].dev : nullptr;
    host.tt_stats_out = tt_stats_bytes ? io.tt_stats[par].dev : nullptr;
    // (the optional outputs of this set were last read by the download of the call three back: same event as the waveforms)
    rc = synthesize_impl(h, set, io.ids[par].dev, B, Ts, sp, nullptr, io.wav[par].dev, nullptr, want_ali ? io.ali[par].dev : nullptr,
                         want_lin ? io.lin[par].dev : nullptr, host);
    if (rc) return rc;
    io.enc_format[par] = -1;
    if (encoded) {
        // behind the call's last stage on its stream: the lengths are the host's already (synth_main has read them)
        std::vector<int32_t>& held = io.enc_held[par];
        held.assign((size_t)B, (int32_t)N_rows);
        const bool ragged = set.eos.enabled != 0;
        if (ragged)
            for (int b = 0; b < B; ++b) held[(size_t)b] = sp->hop_length * (h->eos.last[(size_t)b] - 1);
        const float* rows = io.wav[par].dev;
        if (resampled) {
            float* dst = coded ? rs_rows : reinterpret_cast<float*>(io.codes[par].dev);
            if ((rc = resample_impl(h, rows, B, (int)N_rows, ragged ? held.data() : nullptr, set.out.ratio, (int)N_enc, nullptr, dst))) return rc;
            for (int b = 0; b < B; ++b) held[(size_t)b] = (int32_t)resampled_length(held[(size_t)b], set.out.ratio);
            rows = dst;
        }
        if (coded && (rc = encode_impl(h, rows, B, (int)N_enc, ragged ? held.data() : nullptr, set.out.format, set.out.dither, sp->seed,
                                       io.codes[par].dev, io.enc_stats[par].dev)))
            return rc;
        io.enc_format[par] = set.out.format;
        io.enc_N[par] = (int)N_enc;
        io.enc_B[par] = B;
        io.enc_bytes[par] = code_bytes;
        io.enc_records[par] = coded;
    }
    HIPCHK(h, io.ready[par].record(h->stream));
    HIPCHK(h, io.ready[par].wait(io.out));
    if (encoded) {
        HIPCHK(h, hipMemcpyAsync(io.codes[par].pinned, io.codes[par].dev, code_bytes, hipMemcpyDeviceToHost, io.out));
        if (coded) HIPCHK(h, hipMemcpyAsync(io.enc_stats[par].pinned, io.enc_stats[par].dev, rec_bytes, hipMemcpyDeviceToHost, io.out));
    } else {
        HIPCHK(h, hipMemcpyAsync(io.wav[par].pinned, io.wav[par].dev, n_wav * sizeof(float), hipMemcpyDeviceToHost, io.out));
    }
    if (want_lin) HIPCHK(h, hipMemcpyAsync(io.lin[par].pinned, io.lin[par].dev, n_lin * sizeof(float), hipMemcpyDeviceToHost, io.out));
    if (want_ali) HIPCHK(h, hipMemcpyAsync(io.ali[par].pinned, io.ali[par].dev, n_ali * sizeof(float), hipMemcpyDeviceToHost, io.out));
    if (stats_bytes) HIPCHK(h, hipMemcpyAsync(io.stats[par].pinned, io.stats[par].dev, stats_bytes, hipMemcpyDeviceToHost, io.out));
    if (tt_start_bytes) {
        HIPCHK(h, hipMemcpyAsync(io.tt_start[par].pinned, io.tt_start[par].dev, tt_start_bytes, hipMemcpyDeviceToHost, io.out));
        HIPCHK(h, hipMemcpyAsync(io.tt_stats[par].pinned, io.tt_stats[par].dev, tt_stats_bytes, hipMemcpyDeviceToHost, io.out));
    }
    io.n_stats[par] = stats_bytes ? B : 0;
    io.n_tt[par] = tt_start_bytes ? B : 0;
    io.tt_Ts[par] = Ts;
    io.n_lin[par] = n_lin;
    io.n_ali[par] = n_ali;
    io.frames[par] = h->eos.last;   // (the call has read them: synth_main)
    // the sticky status words of the persistent kernels travel with the waveforms (tts_wait_host must not wait for
    // anything but this call: a stream synchronisation there would wait for the NEXT call's download as well)
    io.status_pinned[2 * par] = io.status_pinned[2 * par + 1] = 0;
    io.failed[par] = false;   // (the set is reused: the ticket that failed can no longer be waited on)
    if (h->pd_used && h->pd_sync)
        HIPCHK(h, hipMemcpyAsync(&io.status_pinned[2 * par + 1], pd_status_word(h), sizeof(int), hipMemcpyDeviceToHost, io.out));
    HIPCHK(h, io.d2h[par].record(io.out));
    io.n_floats[par] = n_wav;
    *ticket = t;
    return TTS_OK;
}


// What every tts_wait_host* call does first: the ticket's range, the host's wait for its download, the decoder's status
static int wait_host_ticket(tts_handle_t h, int ticket) {
    auto& io = h->hio;
    if (ticket < 0 || ticket >= io.tickets || ticket < io.tickets - 3)
        return fail(h, TTS_ERR_INVALID, "wait_host: this ticket's buffer has been handed to a later call (at most three calls in flight)");
    const int par = ticket % 3;
    // (disarmed by a growth of the staging buffers in between: everything was synchronised there, nothing is left to wait for)
    HIPCHK(h, io.d2h[par].sync());
    // the download is behind everything the call launched: a timed-out persistent kernel must not pass for a result
    if (io.status_pinned[2 * par + 1] || io.failed[par]) {
        // what check_status does at a synchronisation, on the first report: the sticky device word is cleared (behind the
        // downloads already queued: a call in flight behind this one may still be reported once, conservatively), the
        // handle leaves the persistent path by itself and stops carrying the word along.  The buffer set stays marked:
        // a second wait on this ticket (tts_wait_host after a failed tts_wait_host_outputs) must not hand out its waveforms
        if (!io.failed[par]) {
            io.failed[par] = true;
            io.status_pinned[2 * par + 1] = 0;
            if (h->pd_sync) HIPCHK(h, hipMemsetAsync(pd_status_word(h), 0, sizeof(int), io.out));
            h->persistent_decoder = 0;
            h->pd_used = false;
        }
        return pd_timed_out(h);
    }
    return TTS_OK;
}


int tts_wait_host(tts_handle_t h, int ticket, const float** wav_host, size_t* n_floats) {
    DeviceScope dev_scope(h);
    if (!h || !wav_host) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);
    if (rc) return rc;
    auto& io = h->hio;
    const int par = ticket % 3;
    if (io.enc_format[par] >= 0)
        return fail(h, TTS_ERR_INVALID, "wait_host: this ticket's call was made with tts_set_output on: its codes are fetched with tts_wait_host_encoded");
    *wav_host = io.wav[par].pinned;
    if (n_floats) *n_floats = io.n_floats[par];
    return TTS_OK;
}


int tts_wait_host_encoded(tts_handle_t h, int ticket, const void** data, size_t* bytes, int* format, int* N_out, const int32_t** n_samples,
                          const tts_encode_stats_t** stats, int* B) {
    DeviceScope dev_scope(h);
    if (!h || !data) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);
    if (rc) return rc;
    auto& io = h->hio;
    const int par = ticket % 3;
    if (io.enc_format[par] < 0)
        return fail(h, TTS_ERR_INVALID, "wait_host_encoded: this ticket's call was made with tts_set_output off: its waveforms are fetched with tts_wait_host");
    *data = io.codes[par].pinned;
    if (bytes) *bytes = io.enc_bytes[par];
    if (format) *format = io.enc_format[par];
    if (N_out) *N_out = io.enc_N[par];
    if (n_samples) *n_samples = io.enc_held[par].data();
    if (stats) *stats = io.enc_records[par] ? io.enc_stats[par].pinned : nullptr;
    if (B) *B = io.enc_B[par];
    return TTS_OK;
}


int tts_wait_host_outputs(tts_handle_t h, int ticket, const float** linear_host, size_t* n_linear, const float** align_host,
                          size_t* n_align) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);   // same event, same checks (ticket range, decoder status)
    if (rc) return rc;
    auto& io = h->hio;
    const int par = ticket % 3;
    if (linear_host) *linear_host = io.n_lin[par] ? io.lin[par].pinned : nullptr;
    if (n_linear) *n_linear = io.n_lin[par];
    if (align_host) *align_host = io.n_ali[par] ? io.ali[par].pinned : nullptr;
    if (n_align) *n_align = io.n_ali[par];
    return TTS_OK;
}


int tts_wait_host_frames(tts_handle_t h, int ticket, const int32_t** n_frames, int* B) {
    DeviceScope dev_scope(h);
    if (!h || !n_frames) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);   // same event, same checks (ticket range, decoder status)
    if (rc) return rc;
    const auto& f = h->hio.frames[ticket % 3];
    *n_frames = f.data();
    if (B) *B = (int)f.size();
    return TTS_OK;
}


int tts_wait_host_alignment_stats(tts_handle_t h, int ticket, const tts_alignment_stats_t** stats, int* B) {
    DeviceScope dev_scope(h);
    if (!h || !stats) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);   // same event, same checks (ticket range, decoder status)
    if (rc) return rc;
    const auto& io = h->hio;
    const int par = ticket % 3;
    if (!io.n_stats[par]) return fail(h, TTS_ERR_INVALID, "wait_host_alignment_stats: this ticket's call was not made with tts_set_alignment_stats on");
    *stats = io.stats[par].pinned;
    if (B) *B = io.n_stats[par];
    return TTS_OK;
}


int tts_wait_host_token_times(tts_handle_t h, int ticket, const int32_t** start, const tts_token_times_stats_t** stats, int* B, int* Ts) {
    DeviceScope dev_scope(h);
    if (!h || !start || !stats) return TTS_ERR_INVALID;
    const int rc = wait_host_ticket(h, ticket);   // same event, same checks (ticket range, decoder status)
    if (rc) return rc;
    const auto& io = h->hio;
    const int par = ticket % 3;
    if (!io.n_tt[par]) return fail(h, TTS_ERR_INVALID, "wait_host_token_times: this ticket's call was not made with tts_set_token_times on");
    *start = io.tt_start[par].pinned;
    *stats = io.tt_stats[par].pinned;
    if (B) *B = io.n_tt[par];
    if (Ts) *Ts = io.tt_Ts[par];
    return TTS_OK;
}


int tts_decoder_kernel_choice(tts_handle_t h, int B, int Ts, int pipelined) {
    if (!h || B < 1 || Ts < 1) return TTS_ERR_INVALID;
    if (!h->finalized) return fail(h, TTS_ERR_NOT_LOADED, "decoder_kernel_choice: weights not finalised");
    return pd_choice(h, B, Ts, pipelined ? h->reserve_cus : h->n_cus_dev, pipelined != 0);
}

}  // extern "C"
