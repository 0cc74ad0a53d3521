// Internals shared by the four translation units of the C ABI (api_handle.hip: handle, workspace allocator, weights, options;
// api_stages.hip: the network's stage entry points and what they enqueue; api_griffin_lim.hip: Griffin-Lim's and the analysis
// side's host code; api_pipeline.hip: tts_synthesize and its host-memory form, the scheduler of the three streams).  Not part of
// the interface: include/sstts_hip.h is.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <utility>
#include <vector>
#include "decoder.h"
#include "decoder_cluster.h"
#include "griffin_lim.h"
#include "synth_plan.h"
#include "tts_common.h"
#include <algorithm>
#include <map>

namespace tts_api {
using namespace tts;


// Upper bounds of tts_config_t that tts_create holds (include/sstts_hip.h documents them per field)
constexpr int TTS_MAX_N_MELS = 1024;                          // floats of the arena's zero block: the decoder's GO frame is read from it
constexpr int TTS_MAX_FIELD = 1 << 20;                        // any count or width: products of three fields fit 64 bits
constexpr long long TTS_MAX_WEIGHT_FLOATS = (1ll << 30) - 5;  // launch_gemm (gemm_f32.hip): 4 N K < 0xFFFFFFF0 bytes per operand

extern thread_local std::string g_create_error;   // tts_create failures (no handle to keep the message in)

struct ManifestEntry {
    std::string name;
    std::vector<int64_t> shape;
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};

struct CbhgWeights {
    int n_banks = 0, n_filters = 0, c_in = 0, proj_filters[2] = {0, 0};
    // device pointers into the arena
    std::vector<const float*> bank_wt, bank_b, bank_scale, bank_shift;
    const float* proj_wt[2];
    const float* proj_b[2];
    const float* proj_scale[2];
    const float* proj_shift[2];
    const float* lifter_wt;
    const float* lifter_b;
    std::vector<const float*> hw_wt, hw_b;
    const float* gru_in_wt;   // [2*3H][units]
    const float* gru_in_b;    // [2*3H]
    const float* gru_rec;     // packed recurrent weights, both directions
};

enum Stage { ST_ENCODER = 0, ST_DECODER, ST_POSTNET, ST_DENORM, ST_GL_ITER, ST_GL_FINAL, ST_DEBUG_GEMM, ST_EVAL_LOSS, ST_FEATURES, ST_SPEECH_END, ST_STRETCH, ST_RESAMPLE, ST_PHASE_INIT, ST_MFCC, ST_DTW, ST_F0, ST_LOUDNESS, ST_ALIGNMENT, ST_JOIN, ST_LIMITER, ST_ENCODE, ST_WARP, ST_SHIFT, ST_EQUALIZE, ST_COMPRESS, ST_WATERMARK, ST_STOI, ST_COUNT };
extern const char* const kStageNames[ST_COUNT];

struct ProfSpan {
    hipEvent_t a, b;
    int stage;
    int64_t launches;
};

// One ordering edge between streams (or a stream and the host): an event and whether something recorded in it still has to be
// waited for.  Created at the first record -- never under a stream capture: nothing records a Signal inside one.
struct Signal {
    hipEvent_t ev = nullptr;
    bool armed = false;
    Signal() = default;
    Signal(const Signal&) = delete;
    Signal& operator=(const Signal&) = delete;
    ~Signal() {
        if (ev) hipEventDestroy(ev);
    }
    hipError_t record(hipStream_t s) {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        if (e == hipSuccess) armed = true;
        return e;
    }
    hipError_t wait(hipStream_t s) const { return armed ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }   // (a stream waits)
    hipError_t sync() const { return armed ? hipEventSynchronize(ev) : hipSuccess; }                     // (the host waits)
    bool done() const { return !armed || hipEventQuery(ev) == hipSuccess; }                              // (nobody waits)
    void disarm() { armed = false; }   // what was recorded is known to be complete, or has been waited for by all it concerns
};

// The run tables of the streaming Griffin-Lim kernel, owned by the handle: one entry per cut (gl_plan in api_griffin_lim.hip makes
// and finds them; DESIGN.md 4.5 has the rules).  A call that finds its cut allocates, copies and waits for nothing; a new one
// costs one asynchronous copy on the call's stream and at most one hipMalloc.  The least recently used entry is replaced: two
// per shape (a pipelined call's narrow and wide cut) for the shapes a server runs; a dataset's length vectors come and go.
constexpr int GL_PLAN_CAPACITY = 16;
struct GlPlanStore {
    struct Entry {
        std::vector<int> key;        // empty: no cut
        std::vector<GlItem> items;   // host copy
        int slots = 1, workers = 1;
        int4* dev = nullptr;         // device table
        size_t room = 0;             // ... and the items it has room for
        // the stream the upload and the launches that read the table are enqueued on (null: nothing since the handle was last
        // synchronised); `ready`: behind the upload -- and behind the readers on the stream before, once it has changed
        hipStream_t stream = nullptr;
        Signal ready;
        unsigned long long used = 0;
    };
    std::vector<std::unique_ptr<Entry>> entries;   // at most GL_PLAN_CAPACITY
    unsigned long long clock = 0;
    // what a replaced entry left behind while enqueued work may still have read it: freed where the handle is synchronised
    std::vector<void*> retired_dev;
    std::vector<std::vector<GlItem>> retired_host;
    void synced();    // every stream of the handle has been synchronised (sync_all)
    void release();   // tts_destroy
};

// Griffin-Lim's work counters (the streaming family of gl_run): a ring of slots, zeroed once; a launch takes the next slot and
// zeroes its predecessor's
constexpr unsigned GL_RING = 256;
struct GlCounterRing {
    unsigned* ring = nullptr;      // the buffer the bookkeeping refers to
    unsigned seq = 0;
    unsigned* last = nullptr;      // slot of the most recent launch (dirty)
    hipStream_t stream = nullptr;
    hipError_t start(unsigned* buf, hipStream_t on);   // starts over where the buffer (a re-allocated workspace) or the stream changed
    void next(GlParams& q);                            // q's launch takes the next slot and zeroes the one before
};

// A pinned host buffer and the device buffer it is copied to or from (tts_synthesize_host); sizes only increase.
template <class T>
struct StagedBuf {
    T* pinned = nullptr;
    T* dev = nullptr;
    size_t bytes = 0;
    StagedBuf() = default;
    StagedBuf(const StagedBuf&) = delete;
    StagedBuf& operator=(const StagedBuf&) = delete;
    ~StagedBuf() { release(); }
    hipError_t release() {
        const hipError_t e1 = pinned ? hipHostFree(pinned) : hipSuccess;
        const hipError_t e2 = dev ? hipFree(dev) : hipSuccess;
        pinned = dev = nullptr;
        bytes = 0;
        return e1 != hipSuccess ? e1 : e2;
    }
    hipError_t grow(size_t need) {   // (the caller has synchronised everything that may still use the buffers)
        if (need <= bytes) return hipSuccess;
        hipError_t e = release();
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&pinned), need, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dev), need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
};

// What tts_synthesize hands to its encoder and decoder per call (encoder_impl / decoder_impl are enqueued on h->stream and take
// everything else from here); default-constructed: a stand-alone call of a stage entry point.  Two instances per call:
// tts_synthesize_host fills `upload` and `enc_done` only, tts_synthesize reads those and fills the rest for decoder_impl.
struct StageArgs {
    int* hold_flag = nullptr;        // the sleepers' flag: a persistent decoder releases the held compute units once resident
    int cu_budget = 0;               // the compute units the front stream may count on (0 = the whole chip, not pipelined)
    bool chip_idle = false;          // the main stream had nothing in flight when this call's decoder was enqueued
    // Under the call pipeline the decoder's output projection (y history -> mel, one GEMM) is not issued behind the decoder
    // on the front stream, where it gets the decoder's 32 compute units (0.3 ms), but at the head of the post-net on the
    // main stream (0.03 ms); the y history is then a buffer per call parity.
    bool project_later = false;
    int parity = 0;
    float* keys = nullptr;           // attention keys of the memory the decoder gets, already computed
    // tts_synthesize_host: the ids' upload, enqueued on the encoder's stream in front of the encoder (behind the last record of
    // `enc_done`, recorded in `done`), and a signal recorded behind the encoder
    struct {
        int32_t* dst = nullptr;
        const int32_t* src = nullptr;
        size_t bytes = 0;
        Signal* done = nullptr;
    } upload;
    Signal* enc_done = nullptr;
    // tts_synthesize_host with tts_set_alignment_stats on: where the call's records go on the device (its buffer set's)
    tts_alignment_stats_t* stats_out = nullptr;
    // ... and with tts_set_token_times on: where its start steps and records go
    int32_t* tt_start_out = nullptr;
    tts_token_times_stats_t* tt_stats_out = nullptr;
};

// tts_synthesize pipelining: encoder + decoder (latency bound, few CUs) of call k+1 run on
// `front` while post-net + Griffin-Lim (throughput bound) of call k run on the handle's `stream`.
struct CallPipeline {
    hipStream_t aux = nullptr;      // stream the sleepers run on
    int* hold_flags = nullptr;      // two flag words, alternating per call
    Signal aux_mark;                // the front and encoder streams start behind this point of the main / sleeper stream
    unsigned call_count = 0;
    // The front stream (encoder, decoder, explicit initial phases of the NEXT call beside this call's post-net and Griffin-Lim):
    // greatest priority.  Measured alternatives for the calls of the persistent decoder (which keeps its CUs by being
    // resident): lowest priority was 0.15 ms per step better while the main stream was the longer one and 0.1 ms worse once
    // Griffin-Lim's run cut had given it slack; the main stream's own priority is as good as the greatest in a device-resident
    // loop but HALVES the throughput of tts_synthesize_host -- streams of one priority share a few hardware queues, and with
    // the copy streams of the host path the front stream lands on the main stream's queue.
    hipStream_t front = nullptr;
    // The encoder of a pipelined call runs on a stream of its own (round 4): it depends on the ids only, so it need not
    // queue behind the previous call's decoder on the front stream -- it runs as soon as the decoder of the call TWO back
    // has finished with this parity's `memory` buffer, i.e. one inter-Griffin-Lim gap earlier, and the decoders follow
    // each other back to back (the step was enc + dec = 17.2 ms against 15.6 ms of post-net + Griffin-Lim).
    hipStream_t encs = nullptr;
    Signal enc_ready[2];   // encoder of the last call of this parity done (enc stream)
    Signal dec_done[2];    // decoder of the last call of this parity done (front stream)
    // ... and not before the main stream has reached the post-net of that call (the Griffin-Lim phase before it is over):
    // an encoder let loose during a Griffin-Lim phase gets its compute units one launch boundary at a time (3 ms for 0.75 ms
    // of work) and slows those launches by 15 %; in the gap it shares the chip with the post-net, as before
    Signal gap[2];
    Signal front_done;     // everything of the last pipelined call on the front stream
    Signal post_done[2];   // post-net of the calls of even / odd parity
    bool gl_wide_used[2] = {false, false};   // the Griffin-Lim phase of that parity's last call ends in launches on ALL compute units
    Signal gl_done[2];     // Griffin-Lim of the calls of even / odd parity (its phase buffers are free)
    // encoder + decoder of an UNPIPELINED call or of a stand-alone stage call (they ran on the main stream); disarmed once the
    // front and encoder streams have waited for it
    Signal serial_done;
    unsigned syn_calls = 0;
    // The previous tts_synthesize call: its shape, the frames its Griffin-Lim reconstructed from (T, or what the speaking
    // rate and the pitch made of them) and the resampling ratio of its pitch (0: none).  A call is pipelined from the second
    // of a key on.
    struct SynKey {
        int B = 0, Ts = 0, n_steps = 0, Tg = 0;
        double rho = 0.0;
        bool same_network(int B_, int Ts_, int n_steps_) const { return B == B_ && Ts == Ts_ && n_steps == n_steps_; }
        bool operator==(const SynKey& o) const { return same_network(o.B, o.Ts, o.n_steps) && Tg == o.Tg && rho == o.rho; }
    } syn_prev;
    int last_enc_ahead = -1;        // did the previous PIPELINED call run its encoder ahead on `encs` (1) or on `front` (0)?

    // Every stream has been synchronised (sync_all): nothing recorded so far orders anything any more
    void reset() {
        for (Signal* s : {&aux_mark, &front_done, &serial_done}) s->disarm();
        for (int i = 0; i < 2; ++i) {
            for (Signal* s : {&enc_ready[i], &dec_done[i], &gap[i], &post_done[i], &gl_done[i]}) s->disarm();
            gl_wide_used[i] = false;
        }
    }
    void teardown() {   // (the handle is about to be deleted; the signals go with it)
        for (hipStream_t s : {front, aux})
            if (s) {
                hipStreamSynchronize(s);
                hipStreamDestroy(s);
            }
        if (hold_flags) hipFree(hold_flags);
        if (encs) hipStreamDestroy(encs);
    }
};

// host-memory calls (tts_synthesize_host): pinned staging of the ids, device copies, pinned waveform buffers and the
// device buffers they are copied from, one set per call in flight (ticket mod 3: the device pipeline holds three calls
// at once since round 4 -- encoder of k + 2, decoder of k + 1, Griffin-Lim of k); the ids go up on the stream that
// runs the call's encoder, the outputs come down on one copy stream
struct HostIo {
    hipStream_t out = nullptr;
    StagedBuf<int32_t> ids[3];
    StagedBuf<float> wav[3];
    Signal h2d[3];      // upload of the ids done
    Signal enc[3];      // encoder done with the ids buffer
    Signal ready[3];    // waveforms complete on the device
    Signal d2h[3];      // waveforms have arrived in pinned memory
    size_t n_floats[3] = {0, 0, 0};
    // optional outputs of a host call (tts_synth_params_t::host_outputs): linear spectrograms and alignments
    StagedBuf<float> lin[3], ali[3];
    size_t n_lin[3] = {0, 0, 0}, n_ali[3] = {0, 0, 0};
    std::vector<int32_t> frames[3];   // the lengths of this set's call (tts_wait_host_frames): all T without end-of-speech stopping
    // the alignment statistics of this set's call (tts_set_alignment_stats; tts_wait_host_alignment_stats): the call's kernels
    // write the device side, the download takes it down with the waveforms; n_stats: the call's B, 0 = made with the setting off
    StagedBuf<tts_alignment_stats_t> stats[3];
    int n_stats[3] = {0, 0, 0};
    // the timing marks of this set's call (tts_set_token_times; tts_wait_host_token_times), likewise; n_tt: the call's B, 0 = made
    // with the setting off; tt_Ts: its Ts
    StagedBuf<int32_t> tt_start[3];
    StagedBuf<tts_token_times_stats_t> tt_stats[3];
    int n_tt[3] = {0, 0, 0}, tt_Ts[3] = {0, 0, 0};
    // the delivery format of this set's call (tts_set_output; tts_wait_host_encoded): the codes -- or the resampled float32 rows --
    // and the encoder's records, which travel instead of the float32 rows; enc_format < 0: made with the setting off.  The rows
    // the call synthesises are the set's `wav` as ever; what the resampler makes of them for the encoder is the workspace "out.resampled"
    StagedBuf<unsigned char> codes[3];
    StagedBuf<tts_encode_stats_t> enc_stats[3];
    int enc_format[3] = {-1, -1, -1}, enc_N[3] = {0, 0, 0}, enc_B[3] = {0, 0, 0};
    size_t enc_bytes[3] = {0, 0, 0};
    bool enc_records[3] = {false, false, false};
    std::vector<int32_t> enc_held[3];   // the samples each row holds, at the output rate
    bool failed[3] = {false, false, false};   // this set's call ended on a decoder timeout: EVERY wait on its ticket fails
    int* status_pinned = nullptr;   // [3][2]: the persistent decoder's sticky status word ([.][1]) as it stood behind
                                    // each call's download
    int tickets = 0;

    void reset() {   // everything has been synchronised: the sets are free
        for (int i = 0; i < 3; ++i)
            for (Signal* s : {&h2d[i], &enc[i], &ready[i], &d2h[i]}) s->disarm();
    }
    void teardown() {   // (the staging buffers and the signals go with the handle)
        if (status_pinned) hipHostFree(status_pinned);
        if (out) hipStreamDestroy(out);
    }
};

// The synthesis settings of a handle: what tts_set_end_of_speech, tts_set_speaking_rate, tts_set_pitch, tts_set_loudness,
// tts_set_limiter, tts_set_equalizer, tts_set_compressor, tts_set_watermark, tts_set_alignment_stats, tts_set_token_times, tts_set_output and the options "gl_momentum" / "gl_init" write.  tts_synthesize and tts_synthesize_host take ONE
// copy when the call is made and read nothing but that copy from then on; with every setting off the call enqueues what it
// always did.  (The stand-alone Griffin-Lim calls have no such copy: they read the handle's momentum and start.)
struct SynthSettings {
    struct {
        int enabled = 0;
        float threshold_db = 0.f;
        int keep_frames = 0;
    } eos;
    double speaking_rate = 1.0;   // 1.0 = off
    double pitch_octaves = 0.0;   // 0 = off
    struct {
        bool enabled = false;
        double target_lufs = -23.0;
        double max_peak = 1.0;
        int sampling_rate = 0;
    } loud;
    struct {
        bool enabled = false;
        double ceiling = 1.0;
        int lookahead = 0;
        int oversample = 1;
    } lim;
    // the equaliser (tts_set_equalizer): the sections are the handle's copy
    struct {
        bool enabled = false;
        int n_sections = 0;
        double sos[40] = {};   // [EQ_MAX_SECTIONS][5]
    } eq;
    // the compressor (tts_set_compressor): the parameters are the handle's copy
    struct {
        bool enabled = false;
        tts_compressor_t params = {};
    } cmp;
    // the watermark (tts_set_watermark): the parameters are the handle's copy
    struct {
        bool enabled = false;
        tts_watermark_t params = {};
    } wm;
    struct {
        bool enabled = false;
        int pad_id = 0;
    } ali;
    struct {
        bool enabled = false;
        int pad_id = 0;
        int max_jump = 4;
    } tt;
    // the delivery format of tts_synthesize_host (tts_set_output): enabled = an encoding or a ratio other than 1
    struct {
        bool enabled = false;
        int format = 0;       // TTS_FMT_*
        int dither = 0;       // TTS_DITHER_*
        double ratio = 1.0;   // rate_out / rate_in; 1.0: no resampling
    } out;
    // fast Griffin-Lim: the momentum alpha in thousandths, 0 (default: the reference's plain loop) .. 999; alpha > 0 runs one
    // iteration per launch whatever gl_pair says (gl_stream_kernel, MOM)
    int gl_momentum = 0;
    // how a Griffin-Lim call without explicit `init_phase` starts: 0 (default) = the seed's random phases, 1 = phases estimated
    // from the call's own magnitudes (phase_init.hip) and handed to the launches as an explicit init_phase would be
    int gl_init = 0;
};

}  // namespace tts_api
using namespace tts_api;   // (the handle is a global type: include/sstts_hip.h declares tts_handle_s)

struct tts_handle_s {
    tts_config_t cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // Launch-per-layer decoder: replay the whole loop from one executable hipGraph instead of enqueueing its ~10 launches per
    // step (9.30 against 9.42 ms for 200 steps at B = 64: the dependent launches are GPU-bound at ~4.7 us each).  OFF by default,
    // and REFUSED on a HIP runtime older than the one the library was built and validated with (graph_runtime_ok below).
    // Round 5 saw replays return wrong mel spectrograms "in a long-lived process"; round 6 found what that process had in
    // common: it had imported torch before the library, so the library ran on PyTorch's BUNDLED libamdhip64 (HIP 7.0.51831, same
    // soname) instead of /opt/rocm's 7.2.26015.  On that runtime a cached decoder graph replays wrongly after other work on the
    // handle (tools/graph_probe.py --torch: 5 of 5, garbage of 1e10...1e33 or last-bit differences; whole suite green there with
    // DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, i.e. without the runtime's pre-built AQL packets -- the graph's dec_gemm_kernel nodes use
    // 16 bytes of scratch); the same binary and sequence are right on the 7.2 runtime, graph on, every time
    // (profiles/r06_experiment_hipgraph.txt).
    int use_graph = 0;
    int fused_tail = 1;          // CBHG: lifter + highway stack + GRU input projections as one launch (cbhg_tail.hip)
    bool tail_configured = false;
    int profile = 0;
    int pipeline = 1;      // on while the library owns its stream (see tts_synthesize); ~9 % on MI355X
    int reserve_cus = 32;  // CUs held for the front stream by LDS-hogging sleeper workgroups (reserve.hip)
    int hold_lds_kb = 64;  // LDS of one sleeper: > 80 KB guarantees one sleeper per CU
    int enc_stream = 1;   // option "enc_stream": 0 = the encoder on the front stream in front of its decoder (round 3)
    CallPipeline pl;       // the streams, signals and per-parity state of the call pipeline
    // persistent decoder (decoder_ws.hip / decoder_persistent.hip): 0 never, 2 whenever a kernel covers the configuration,
    // 1 (default) where it was measured to be the faster choice: pd_choice() below has the rule and the numbers.
    int persistent_decoder = 1;
    // which persistent kernel: 1 (default) = the weight-stationary one (decoder_ws.hip: clusters of 16 workgroups x 32
    // utterances, weights in registers) wherever it covers the configuration and its 16 * ceil(B / 32) workgroups fit the
    // budget, else decoder_persistent.hip (8 x 16, weights streamed from L2 every step); 0 = always the latter
    int pd_ws = 1;
    // (the decoder's output projection -- one GEMM over all steps -- runs on the MAIN stream in front of the post-net under the
    //  call pipeline: StageArgs::project_later.  On the front stream behind its decoder it gave the same 14.45 ms per step in
    //  round 5; the option that switched it is gone)
    bool ws_configured = false;
    int gl_pair = 3;                 // Griffin-Lim iterations per launch (1..3) where nothing per-iteration is asked for
    // First Griffin-Lim launch of a pipelined call that is cut for all compute units (gl_run, `wide_from`): -1 = by the rule
    // in gl_wide_from() below, -2 = never, >= 0 = that launch index.
    int gl_wide = -1;
    int n_cus_dev = 0;
    bool pd_configured = false;
    // Test / diagnostic hooks, all per handle and all inert unless the option "debug_hooks" has been set to 1 on THIS handle
    // (include/sstts_hip.h): nothing in the environment and no other handle can change what a call computes.
    int debug_hooks = 0;
    int pd_debug_delay = 0;   // PdParams::dbg_delay: workgroup 3 of every decoder cluster stages late
    int gl_runs = 0;          // Griffin-Lim run cut: runs per utterance (0 = planned)
    int gl_run_len = 0;       // ... or frames per full run (0 = planned)
    int timeline = 0;         // print the absolute stage times of every profiled span (prof_collect)
    int gl_workers = 0;       // Griffin-Lim: plan and launch for this many workgroups (0 = the free compute units)
    GlCounterRing gl_ring;    // Griffin-Lim's work counters
    bool pd_used = false;            // a persistent launch has been enqueued since the last status check
    unsigned* pd_sync = nullptr;     // sync words of the last persistent launch, laid out for pd_clusters (decoder_cluster.h)
    int pd_clusters = 0;
    int pd_rows = 0;                 // tests ("pd_rows" behind "debug_hooks"): utterances per cluster of the weight-stationary decoder, 16 / 32
    int pd_rows_used = 0;            // ... of the last launch

    HostIo hio;   // tts_synthesize_host: staging buffers, copy stream and signals of the three calls in flight

    std::vector<ManifestEntry> manifest;
    std::map<std::string, std::vector<float>> host_w;
    bool finalized = false;

    // device weight arena
    float* arena = nullptr;
    size_t arena_floats = 0;

    const float* embedding = nullptr;
    const float* enc_pre_wt[2];
    const float* enc_pre_b[2];
    CbhgWeights enc, post;
    const float* mem_wt = nullptr;
    DecoderWeights dec;
    const float* dense_wt = nullptr;
    const float* dense_b = nullptr;
    const float* zeros = nullptr;   // TTS_MAX_N_MELS zero floats inside the arena

    // workspace (grow-only); ws_allocs: the allocations ws_get has made -- a caller that reads it around a request knows
    // whether the buffer is new or grew
    std::map<std::string, DevBuf> ws;
    unsigned ws_allocs = 0;

    // decoder graph cache
    hipGraphExec_t dec_graph = nullptr;
    // A launch of dec_graph is complete: recorded behind every hipGraphLaunch, waited for by the HOST before the same
    // executable graph is launched again or destroyed (never two launches of one hipGraphExec_t in flight, never one
    // destroyed under a launch).
    Signal graph_done;
    hipGraph_t dec_graph_src = nullptr;   // the captured graph the executable one was instantiated from: kept alive with it
    struct {   // everything the captured launches have baked in: shapes and EVERY pointer (decoder_impl)
        const void* memory = nullptr;
        const void* keys = nullptr;
        void* align = nullptr;
        int B = 0, Ts = 0, n_steps = 0;
        DecoderScratch sc;
        DecoderWeights w;
    } dec_key;

    // Griffin-Lim tables
    struct {
        int win = 0, hop = 0, T = 0;
        float* window = nullptr;
        float* wss = nullptr;      // reciprocal window sum-square
        float* wlane = nullptr;    // per-lane window images of the Griffin-Lim kernel
        float2* tw1024 = nullptr;
        float2* tw2048 = nullptr;
        float2* tables = nullptr;
        bool configured = false;
    } gl;

    // general power-of-two path (griffin_lim_generic.hip): twiddles per n_fft, window tables of the last configuration
    struct {
        std::map<int, float2*> tw;          // n_fft -> exp(-2 pi i k / n_fft), k < n_fft / 2
        int n_fft = 0, win = 0, hop = 0, T = 0;
        float* window = nullptr;
        float* rwss = nullptr;
        bool configured = false;
    } glg;

    GlPlanStore gl_plans;   // run tables of the streaming kernel, uniform and ragged batches alike

    // ragged Griffin-Lim (tts_griffin_lim_ragged): what the last call uploaded -- the lengths with the window sum-square
    // tables made for them -- kept while the next call asks for the same
    struct {
        std::vector<int> tab_key;
        const int* lens = nullptr; // [B] device (workspace "gl.rag_lens", or the caller's: gl_rag_tables)
        float* rw = nullptr;       // streaming [B][2][rw_E], general [B][n_fft + hop (T_max - 1)] (workspace "gl.rag_rw")
    } rag;

    // the synthesis settings as the tts_set_* calls and the options "gl_momentum" / "gl_init" left them
    SynthSettings settings;

    // end-of-speech stopping: the lengths a call's detection leaves on the device (workspace "eos.frames": one buffer -- the
    // detection and the Griffin-Lim launches that read it follow each other on the main stream, call after call), the pinned
    // words the host reads them from, and the last call's lengths
    struct {
        int32_t* pinned = nullptr;
        int pinned_room = 0;
        std::vector<int32_t> last;
    } eos;

    // attention diagnostics: last_dev / last_B: the records of the last call on the device (null: that call was made with the
    // setting off); done: recorded behind its statistics on the stream its decoder ran on
    struct {
        const tts_alignment_stats_t* last_dev = nullptr;
        int last_B = 0;
        Signal done;
        hipStream_t copy = nullptr;   // tts_synth_alignment_stats and tts_synth_token_times copy on it, behind `done` alone
    } ali;

    // timing marks, likewise: the start steps and records of the last call on the device (null: made with the setting off)
    struct {
        const int32_t* last_start = nullptr;
        const tts_token_times_stats_t* last_stats = nullptr;
        int last_B = 0, last_Ts = 0;
        Signal done;
    } tt;

    // the per-utterance lengths of the last tts_synthesize call (synth_plan.h): Griffin-Lim and the resampler are given them
    SynthLengths syn_lens;

    // the resampler (resample.hip): the half window before a ratio's scale, and the phase-major tables per ratio on the device
    struct {
        std::vector<double> base;
        std::map<uint64_t, double*> tabs;
    } rs;

    // cepstra (cepstrum.hip): the DCT tables on the device, one per (n_mels << 32 | n_mfcc)
    std::map<uint64_t, double*> mfcc_tabs;

    // formant-preserving pitch (shift.hip): the cosine table per N and the lifter per order on the device
    struct {
        std::map<int, double*> ct, lifter;
        bool configured = false;   // the kernel's LDS limit has been raised on this handle's device
    } shift;

    // analysis-side tables (STFT window, mel basis)
    struct {
        int win = 0;
        float* window = nullptr;
        int sr = 0, n_fft = 0, n_mels = 0;
        float fmin = 0, fmax = 0;
        float* mel_wt = nullptr;   // [n_mels][FP]
        int* flag = nullptr;
    } an;

    // dataset feature pass (features.hip): tables of the last configuration, pinned staging of the per-recording descriptors
    struct {
        int n_fft = 0, win = 0;
        float* window = nullptr;          // [win] periodic hann
        int sr = 0, n_mels = 0;
        float fmin = 0, fmax = 0;
        float* mel_w = nullptr;           // packed non-zero filterbank weights
        int* mel_band = nullptr;          // [n_mels][2] {first bin, first weight}, [n_mels] end bins follow
        void* staging = nullptr;          // pinned host buffer of the descriptor uploads
        size_t staging_bytes = 0;
        Signal staged;                    // the last upload from `staging` has been read
    } feat;

    // profiling
    std::vector<ProfSpan> spans;
    double prof_ms[ST_COUNT] = {0};
    int64_t prof_launches[ST_COUNT] = {0};
};


namespace tts_api {

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
            return TTS_ERR_HIP;                                                                 \
        }                                                                                       \
    } while (0)

// Every entry point that takes a handle runs on the handle's device, whatever device is current on the calling
// thread (one process may hold handles on several GPUs, or a caller may have switched devices after tts_create);
// the caller's current device is restored on return.
struct DeviceScope {
    int prev = -1;
    bool changed = false;
    explicit DeviceScope(tts_handle_t h) {
        if (!h) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != h->device) changed = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceScope() {
        if (changed) hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

#define WS(h, name, type, count, var)                                             \
    type* var = nullptr;                                                          \
    {                                                                             \
        void* _p = nullptr;                                                       \
        int _rc = ws_get(h, name, (size_t)(count) * sizeof(type), &_p);           \
        if (_rc != TTS_OK) return _rc;                                            \
        var = reinterpret_cast<type*>(_p);                                        \
    }

// ------------------------------------------------------------------------------------ profiling
struct ProfScope {
    tts_handle_t h;
    int idx = -1;
    ProfScope(tts_handle_t h_, int stage, int64_t launches) : h(h_) {
        if (!h->profile) return;
        ProfSpan s{};
        if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
        s.stage = stage;
        s.launches = launches;
        hipEventRecord(s.a, h->stream);
        h->spans.push_back(s);
        idx = (int)h->spans.size() - 1;
    }
    ~ProfScope() {
        if (idx >= 0) hipEventRecord(h->spans[idx].b, h->stream);
    }
};

// ---- defined in api_handle.hip / api_stages.hip / api_griffin_lim.hip / api_pipeline.hip
int fail(tts_handle_t h, int code, const std::string& msg);
void build_manifest(tts_handle_t h);
int pd_timed_out(tts_handle_t h);   // the persistent decoder's timeout, reported in ONE wording (check_status, tts_wait_host)
int check_status(tts_handle_t h);
inline int* pd_status_word(tts_handle_t h) { return dc_sync(h->pd_sync, h->pd_clusters).status; }   // sticky, on the device
int sync_all(tts_handle_t h);
int graph_quiesce(tts_handle_t h);
int graph_drop(tts_handle_t h);
int ws_get(tts_handle_t h, const char* name, size_t bytes, void** out);
void prof_collect(tts_handle_t h);
void feat_release(tts_handle_t h);   // features.hip: the feature pass's tables and staging
GemmGroup dense_group(const float* A, int lda, const float* Wt, const float* bias, float* C, int ldc, int M, int N, int K, int act);
GemmGroup conv_group(const float* A, int Cin, int ktaps, int T, const float* Wt, const float* bias, const float* scale, const float* shift, float* C, int ldc, int coff, int M, int N, int act, int pool);
int run_single(tts_handle_t h, const GemmGroup& g);
bool graph_runtime_ok(int* have);
int run_cbhg(tts_handle_t h, const CbhgWeights& w, const char* tag, const float* x, int B, int T, float* out, int64_t* launches);
int check_ready(tts_handle_t h);
int gl_tables(tts_handle_t h);
int device_cus(tts_handle_t h);
int gl_fp(int n_fft);
bool gl_is_streaming(int n_fft, int win, int hop);
int glg_twiddles(tts_handle_t h, int n_fft, const float2** out);
int glg_prepare(tts_handle_t h, int T, int win, int hop, int n_fft);
int gl_refuse(tts_handle_t h, const GlRefusal& r);   // gl_refusal's answer (gl_plan.h) as a return code: fail() with its text, or TTS_OK
int gl_prepare(tts_handle_t h, int T, int win, int hop, int n_fft);
// One Griffin-Lim call: what tts_griffin_lim / tts_griffin_lim_ragged and synth_main ask of gl_run, which takes the streaming kernel
// where gl_is_streaming says so and the general kernels elsewhere.  Nothing behind it reads the handle's settings.
struct GlCall {
    const float* mag = nullptr;           // time-major magnitudes [B][T][gl_fp(n_fft)]
    const float* init_ft = nullptr;       // reference-layout U[0,1) numbers, or null: then the seed
    uint64_t seed = 0;
    int B = 0, T = 0, n_iter = 0, win = 0, hop = 0, n_fft = 0;   // T: T_max of a ragged batch
    float *wav = nullptr, *mse = nullptr; // the waveforms; the last iteration's error per utterance, or null
    bool peak_normalize = false;
    const int32_t* n_frames = nullptr;    // a ragged batch: host lengths [B]; null = one length
    const int* d_frames = nullptr;        // the same lengths, already in device memory (null: they are uploaded)
    int momentum = 0;                     // "gl_momentum": alpha in thousandths
    // what only a pipelined call sets (the streaming kernel)
    bool under_reservation = false;       // `reserve_cus` compute units are kept free of Griffin-Lim
    float2* const* phase_pair = nullptr;  // the two phasor-code buffers to iterate in (null: the handle's own pair)
    bool phase_ready = false;             // phase_pair[0] already holds the initial phasors (another stream, the caller's events)
    int wide_from = -1;                   // launches from this index on are cut for ALL compute units (gl_wide_from); -1: none
};
int gl_run(tts_handle_t h, const GlCall& c);
// ---- Workspaces.  A stage's buffers are named in ONE function, `<stage>_scratch`, which takes the shape that decides their sizes and
// fills a struct of typed pointers.  The stage asks it for its pointers; a synthesis call asks it ahead for the same shape, before
// anything of the call is enqueued (synth_workspaces: a workspace that grows synchronises every stream), so the stage finds them in place.
// Griffin-Lim's (api_griffin_lim.hip).  momentum: the handle's or the call's "gl_momentum"; `mom`, the previous projection, exists for a call
// that has a second iteration to use it, and mom_grew says that this request made or enlarged it (what synth_workspaces counts).
struct GlgScratch { float2* phase; float* frames; float* mse_partial; float2* mom; bool mom_grew; };   // the general kernels
int glg_scratch(tts_handle_t h, int B, int T, int win, int n_fft, int momentum, int n_iter, GlgScratch* s);
// The streaming kernel.  mse_partial has a slot per run of an utterance for ANY planned cut of T frames: no run is shorter than half
// a round of the waves (tests/gl_plan_check.cpp holds the planner to it).  min_slots: the cuts in hand, which only a cut forced through
// the debug hooks takes beyond that; frame_mse: the call wants the error, which momentum keeps per frame; own_phase: the handle's
// pair of phasor-code buffers, for a caller that brings none.
struct GlScratch { float2* mom; bool mom_grew; float* mse_partial; unsigned* counter_ring; float2* phase[2]; };
int gl_scratch(tts_handle_t h, int B, int T, int momentum, int n_iter, bool frame_mse, int min_slots, bool own_phase, GlScratch* s);
// A ragged batch's window sum-square rows of `row` floats -- streaming: [2][gl_rw_edge_len], general kernels: n_fft + hop (T_max - 1) --
// and, with own_lens, room for lengths that are not on the device already (gl_rag_tables fills both)
struct RagScratch { float* rw; size_t row; int* lens; };
int gl_rag_scratch(tts_handle_t h, int B, int T_max, int win, int hop, int n_fft, bool streaming, bool own_lens, RagScratch* s);
int gl_mag_scratch(tts_handle_t h, int B, int T, int row_stride, float** mag);   // the time-major magnitudes Griffin-Lim reads
// end of speech (speech_end.hip / api_stages.hip); EosScratch::frames: the lengths on the device, for a synthesis call
struct EosScratch { unsigned char* active; int32_t* frames; };
int eos_scratch(tts_handle_t h, int B, int T, bool with_frames, EosScratch* s);
int speech_threshold(float threshold_db, float ref_db, float max_db, float power, int units, float* out);
int speech_frames_impl(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold, int keep_frames, int min_frames, int32_t* n_frames, int32_t* last_active);
// speaking rate (stretch.hip): both layouts of the time-stretch, arguments checked by the caller (stretch_plan.h)
int stretch_impl(tts_handle_t h, const float* in, int B, int T, int F, int row_stride, bool time_major, const int32_t* n_frames, double rate,
                 int T_out, float* out);
// the resampler (resample.hip): arguments checked by the caller (resample_plan.h).  resample_table makes a ratio's table ahead
// of a call that must not allocate once it has begun to enqueue
int resample_table(tts_handle_t h, double rho, const double** tab);
// loudness (loudness.hip): arguments checked by the caller (loudness_plan.h)
struct LoudScratch { double *ws, *z; unsigned* peak; };   // ws: the measurement's states and sums, loud_ws_doubles(N, sr) per row
int loudness_scratch(tts_handle_t h, int B, int N, int sr, LoudScratch* s);
int loudness_impl(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, int sr, bool normalize, double target_lufs, double max_peak,
                  double* mean_square, int32_t* n_blocks, double* gain);
// the peak limiter (limiter.hip): arguments checked by the caller (limiter_plan.h)
struct LimScratch { float* out; int* flags; tts_limit_stats_t* stats; };   // the limited copy of the rows, a flag per tile of a row
int limiter_scratch(tts_handle_t h, int B, int N, LimScratch* s);
int limiter_impl(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, double ceiling, int lookahead, int oversample,
                 tts_limit_stats_t* stats);
// the equaliser (equalizer.hip): arguments checked by the caller (equalizer_plan.h)
struct EqScratch { double *state, *M; };   // the segments' states [B][2 S][segments], the transition [2 S][2 S]
int equalizer_scratch(tts_handle_t h, int B, int N, int n_sections, EqScratch* s);
int equalizer_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const double* sos, int n_sections);
// the compressor (compressor.hip): arguments checked by the caller (compressor_plan.h)
struct CmpScratch { double* state; void* partial; };   // the segments' states [B][2][segments]; pass C's records [B][tiles], where asked for
int compressor_scratch(tts_handle_t h, int B, int N, bool records, CmpScratch* s);
int compressor_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_compressor_t& params,
                    double* envelope, tts_compress_stats_t* stats);
// the watermark's embedder (watermark.hip): arguments checked by the caller (watermark_plan.h)
struct WmScratch { float* E; void* partial; };   // the blocks' maxima [B][blocks]; the tiles' records [B][tiles], where asked for
int watermark_scratch(tts_handle_t h, int B, int N, bool records, WmScratch* s);
int watermark_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_watermark_t& params,
                   tts_watermark_embed_stats_t* stats);
// intelligibility (stoi.hip): the frame energies, the segments' sums and degenerate counts [B][frames]; the kept frames' indices
// [B][frames] and the envelopes [B][2][15][frames] where the caller brings no room for them
struct StoiScratch { double *energy, *sums; int32_t* degs; int32_t* index; double* env; };
int stoi_scratch(tts_handle_t h, int B, int N, bool own_index, bool own_envelopes, StoiScratch* s);
// the delivery encoder (encode.hip): arguments checked by the caller (encode_plan.h).  The records of a call that takes none
struct EncScratch { tts_encode_stats_t* stats; };
int encode_scratch(tts_handle_t h, int B, EncScratch* s);
int encode_impl(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, int format, int dither, uint64_t seed, void* out,
                tts_encode_stats_t* stats);
// attention diagnostics (alignment.hip): arguments checked by the caller (alignment_plan.h); d_n_sent: the sentence lengths on the
// device, or null.  Two sets of scratch: the stand-alone entry point runs on the main stream, the statistics of a synthesis call
// (in_call) behind its decoder -- under the call pipeline on the front stream -- and nothing orders the one behind the other.
struct AlignScratch { int32_t* pos; float* peak; unsigned char* off; int32_t* dur; };
int alignment_scratch(tts_handle_t h, bool in_call, int B, int n_steps_max, int Ts, AlignScratch* s);
int alignment_impl(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                   const int32_t* d_n_sent, tts_alignment_stats_t* stats, int32_t* durations, int32_t* pos, float* peak);
int alignment_positions_impl(tts_handle_t h, bool in_call, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent,
                             const int32_t* n_steps, const int32_t* d_n_sent, bool run, const int32_t** pos);
// timing marks (token_times.hip): arguments checked by the caller (token_times_plan.h); d_n_sent and the two sets of scratch as
// above.  start, stats: a synthesis call's results where its caller gave no room for them (null in the stand-alone set)
struct TokenTimesScratch { int32_t* path; unsigned char* dir; int32_t* start; tts_token_times_stats_t* stats; };
int token_times_scratch(tts_handle_t h, bool in_call, int B, int n_steps_max, int Ts, TokenTimesScratch* s);
int token_times_impl(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                     const int32_t* d_n_sent, bool have_pos, int max_jump, int32_t* start, int32_t* path, tts_token_times_stats_t* stats);
int text_lengths_impl(tts_handle_t h, const int32_t* ids, int B, int Ts, int pad_id, int32_t* n_sent);
int resample_impl(tts_handle_t h, const float* wav, int B, int n, const int32_t* n_samples, double rho, int N_out, const int32_t* keep_cap,
                  float* out);
void resample_release(tts_handle_t h);
void mfcc_release(tts_handle_t h);   // cepstrum.hip: the DCT tables
void shift_release(tts_handle_t h);  // shift.hip: the cosine tables and lifters
// estimated initial phases (phase_init.hip): both input layouts -> the public (B, F, T) array on h->stream, arguments checked by
// the caller (phase_plan.h).  gl_init_phase: the init_phase of a Griffin-Lim call -- the caller's, or with gl_init (the option "gl_init" of the handle or the call) the
// estimate from the time-major magnitudes `magi` in PhaseScratch::init_est, or null.
// mag_rows: from_public alone (the (B, F, T) input, transposed); the three chunk maps: with more than one chunk of frames alone;
// init_est: gl_start alone, the estimate as the public-layout init_phase of a Griffin-Lim call
struct PhaseScratch { float *u_rows, *mag_rows; unsigned short* map_s; unsigned *map_o, *start; float* init_est; };
int phase_estimate_scratch(tts_handle_t h, int B, int T, int n_fft, bool from_public, bool gl_start, PhaseScratch* s);
int phase_estimate_impl(tts_handle_t h, const float* mag, int B, int T, int row_stride, bool time_major, const int32_t* n_frames, int n_fft,
                        int hop, float* out);
int gl_init_phase(tts_handle_t h, int gl_init, const float* magi, const float* init_phase, int B, int T, int row_stride, const int32_t* n_frames,
                  int n_fft, int hop, const float** out);
int standalone_begin(tts_handle_t h);
int standalone_end(tts_handle_t h);
int encoder_impl(tts_handle_t h, const int32_t* ids, int B, int Ts, float* memory);
int pd_kernel_for(tts_handle_t h, int B, int Ts, int budget);
int pd_choice(tts_handle_t h, int B, int Ts, int budget, bool pipelined);
int attention_keys(tts_handle_t h, const float* memory, int B, int Ts, float* keys);
int teacher_choice(tts_handle_t h, int B, int Ts);
int decoder_impl(tts_handle_t h, const float* memory, int B, int Ts, int n_steps, float* mel, float* alignments,
                 const float* target = nullptr, const StageArgs& args = StageArgs(), std::optional<GemmGroup>* deferred = nullptr);
int postnet_impl(tts_handle_t h, const float* mel, int B, int T, float* linear, float* mag, float ref_db, float max_db, float power, int* db_flag = nullptr);
bool denorm_can_assert(float ref_db, float max_db);
int denorm_flag_arm(tts_handle_t h, int** flag);
int denorm_flag_read(tts_handle_t h);
int gl_wide_from(tts_handle_t h, const SynthSettings& set, int B, int Ts, int n_steps, int T, int n_iter);

}  // namespace tts_api
