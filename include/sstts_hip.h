/*
 * sstts_hip.h -- C ABI of the MI355X-native Tacotron inference hot path.
 *
 * One shared library (libsstts_hip.so, hand-written HIP for gfx950), plain pointers and
 * sizes, no C++/torch types.  The reference (yweweler/single-speaker-tts) has no FFI: its
 * boundary is the Python module surface of tacotron.model / tacotron.inference /
 * audio.synthesis / audio.conversion / audio.features.  Each entry point below names the
 * reference interface (file:line under the reference tree) whose arithmetic it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers (HIP), float32 row-major, batch-major,
 *     channels-last unless stated; ids are int32.  The caller owns every in/out buffer;
 *     the library owns weights and scratch inside the handle.  tts_malloc/tts_memcpy_* let
 *     a host without any other GPU runtime (plain ctypes + numpy) drive the library.
 *   - Every function returns 0 on success or a negative tts_status code and never throws.
 *     tts_last_error(handle) returns a human-readable description of the last failure.
 *   - A handle is bound to one device and one stream; calls on one handle must be
 *     serialised by the caller.  Distinct handles (one per GPU / process) are independent:
 *     every entry point that takes a handle switches to the handle's device for the call and
 *     restores the caller's current device on return.
 *   - Calls are asynchronous on the handle's stream unless stated; tts_synchronize waits.
 *   - Same inputs (and the same init_phase / seed) give bit-identical outputs run to run:
 *     every reduction has a fixed order, no float atomics are used.
 */
#ifndef SSTTS_HIP_H
#define SSTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tts_handle_s* tts_handle_t;

enum tts_status {
    TTS_OK = 0,
    TTS_ERR_INVALID = -1,      /* bad argument / shape */
    TTS_ERR_NOT_LOADED = -2,   /* weights missing or not finalised */
    TTS_ERR_HIP = -3,          /* HIP runtime error */
    TTS_ERR_DB_RANGE = -4,     /* dB < -100: reference audio/conversion.py:47-49 AssertionError */
    TTS_ERR_UNSUPPORTED = -5   /* configuration outside what the kernels implement */
};

/* Architecture hyper-parameters; field names and defaults follow the reference's
 * model_params (tacotron/params/model.py:8-153).  ALWAYS start from tts_default_config: it fills the defaults and
 * `struct_size`, and tts_create refuses a struct whose size is not the library's (a caller built against another version of
 * this header, or a zero-initialised struct) instead of reading past its end or taking zeros for settings.
 *
 * Accepted range of every field (anything else: TTS_ERR_UNSUPPORTED / TTS_ERR_INVALID from tts_create, before the device is
 * touched; the message names the limit).  Common to all counts and widths: at most 2^20; and every weight matrix a GEMM
 * loader reads -- the embedding table, the pre-nets, a bank convolution, a projection, the output projection -- holds at
 * most 2^30 - 5 floats (32-bit byte offsets).  tests/test_gpu_architectures.py runs the network against the float64 oracle
 * at architectures that move every one of these fields (tests/arch_cases.py).
 * Decoder form: the persistent kernels (option "persistent_decoder") cover 2 decoder GRU layers, dec_prenet_units
 * {256, 128} and n_mels <= 256 (the streamed-weights kernel also needs n_mels % 16 == 0, which tts_create demands anyway);
 * every other accepted architecture takes one launch per layer, whatever the option says.  CBHG tail: the fused launch
 * (option "fused_tail") covers an input of at most 128 channels (enc_prenet_units[1], n_mels) and at most 8 highway layers;
 * wider or deeper ones run layer by layer, with the same result to rounding. */
typedef struct tts_config {
    int32_t struct_size;         /* sizeof(tts_config_t) of the header the caller was built with (set by tts_default_config) */
    int32_t vocabulary_size;     /* 39: >= 1 */
    int32_t embedding_size;      /* 256: a multiple of 16 */
    int32_t enc_prenet_units[2]; /* 256, 128: multiples of 16 */
    int32_t enc_n_banks;         /* 16: >= 1 (more than 16 banks: several launches) */
    int32_t enc_n_filters;       /* 128: a multiple of 32 */
    int32_t enc_proj_filters[2]; /* 128, 128 (kernel size 3; relu, linear): [0] a multiple of 4, [1] == enc_prenet_units[1] (residual) */
    int32_t post_n_banks;        /* 8: >= 1 */
    int32_t post_n_filters;      /* 128: a multiple of 32 */
    int32_t post_proj_filters[2];/* 256, 80: [0] a multiple of 4, [1] == n_mels (residual) */
    int32_t n_highway_layers;    /* 4: >= 0 */
    int32_t n_highway_units;     /* 128, nothing else */
    int32_t n_gru_units;         /* 128, nothing else (CBHG bi-GRU, both encoder and post-net) */
    int32_t dec_prenet_units[2]; /* 256, 128: multiples of 16 */
    int32_t n_attention_units;   /* 256, nothing else */
    int32_t n_decoder_gru_units; /* 256, nothing else */
    int32_t n_decoder_gru_layers;/* 2: 1 .. 4 */
    int32_t n_mels;              /* 80: a multiple of 16, at most 1024 (the GO frame is read from a block of 1024 zeros) */
    int32_t reduction;           /* 5: >= 1 (256 x n_mels x reduction within the weight limit) */
    int32_t n_fft;               /* 2048 */
    int32_t force_cudnn;         /* 0: tf GRUCell (TF-CPU parity target); 1: CudnnCompatibleGRUCell */
    /* model_params.attention (tacotron/params/model.py:112-128).  The local mechanism is the reference's
     * experimental LocalLuongAttention (tacotron/attention.py:109-342) in its default sub-mode:
     * AttentionMode.MONOTONIC or PREDICTIVE with AttentionScore.DOT; GENERAL / CONCAT raise NotImplementedError
     * in the reference. */
    int32_t attention_mechanism; /* TTS_ATTENTION_LUONG (default) | TTS_ATTENTION_LOCAL_LUONG */
    int32_t luong_local_window_d;/* 10: window = 2D+1 memory positions around the decoder step index */
    int32_t luong_force_gaussian;/* 1: reported alignments are gaussian-weighted (attention.py:73-80) */
    int32_t luong_local_mode;    /* TTS_LOCAL_MONOTONIC (default): window centre = decoder step index, clamped into
                                  * the memory; TTS_LOCAL_PREDICTIVE: centre p = T_s sigmoid(v_p^T tanh(W_p h)) per
                                  * utterance (attention.py:246-258), two more weights in the manifest.  A predicted
                                  * window that leaves the memory makes tts_decoder_forward / tts_synthesize return
                                  * TTS_ERR_UNSUPPORTED (the reference fails at run time there, attention.py:288-304);
                                  * in this mode those calls synchronise the stream to read that condition. */
    int32_t apply_post_processing;/* 1 (default): post-net CBHG in front of the final Dense; 0: the final Dense straight on the
                                  * mel spectrogram, manifest entry dense/kernel (n_mels, 1 + n_fft / 2) and no post_process/...
                                  * weights (reference tacotron/model.py:388-391, params/model.py apply_post_processing) */
} tts_config_t;

enum tts_attention { TTS_ATTENTION_LUONG = 0, TTS_ATTENTION_LOCAL_LUONG = 1 };
enum tts_local_mode { TTS_LOCAL_MONOTONIC = 0, TTS_LOCAL_PREDICTIVE = 1 };

/* ---- lifecycle ------------------------------------------------------------------------ */
const char* tts_version(void);
int tts_default_config(tts_config_t* cfg);
/* Replaces graph construction `Tacotron(inputs, Mode.PREDICT)` (tacotron/model.py:35-112). */
int tts_create(const tts_config_t* cfg, int device_id, tts_handle_t* out);
int tts_destroy(tts_handle_t h);
const char* tts_last_error(tts_handle_t h);        /* h may be NULL: last create-time error */
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream. */
int tts_set_stream(tts_handle_t h, void* hip_stream);
/* Options: "use_graph" (launch-per-layer decoder loop replayed from a hipGraph; default 0; 1 is refused with
 * TTS_ERR_UNSUPPORTED when the process runs the library on a HIP runtime older than the one it was built with -- a host that
 * loads another ROCm's libamdhip64 first, e.g. by importing torch, serves the library with that one, and graph replays were
 * wrong on PyTorch's bundled 7.0 runtime; see csrc/api_internal.h, `use_graph`), "profile" (record
 * per-stage HIP events, default 0), "pipeline" (default 1: tts_synthesize runs the encoder and
 * the decoder loop of a call on a second stream so that they overlap the Griffin-Lim iterations of
 * the PREVIOUS call still in flight; inputs must be complete when the call is made, which is why 1 applies
 * only while the library owns its stream -- 2 pipelines on a stream adopted with tts_set_stream as well, the
 * caller vouching for its inputs), "reserve_cus" (default 32: compute units kept free of
 * Griffin-Lim workgroups for that second stream, 0 = none), "hold_lds_kb" (default 64: LDS one sleeper workgroup
 * of that reservation allocates), "persistent_decoder" (the whole decoder loop as ONE launch of co-resident
 * workgroup clusters; two decoder GRU layers, layer widths of the reference: 1 (default) = the weight-stationary kernel
 * wherever it covers the configuration and its workgroups fit -- pipelined calls of up to 64 utterances, unpipelined calls of
 * up to 512 -- with 16 or 32 utterances per cluster of 16 compute units as the free units allow (the same bits either way,
 * so a call's spectrograms do not depend on what the handle ran before); 2 = any persistent kernel whenever the configuration
 * allows; 0 = never: one launch per layer; tts_synchronize reports TTS_ERR_HIP if one of its bounded waits timed out),
 * "gl_pair" (Griffin-Lim iterations per launch, 1..3, default 3: the spectrum passes from one iteration to the next in
 * registers; identical arithmetic per iteration), "gl_momentum" (fast Griffin-Lim, Perraudin / Balazs / Soendergaard 2013: the
 * momentum alpha in thousandths, 0 .. 999, default 0 = the reference's plain loop; any other value is TTS_ERR_INVALID and
 * leaves the option as it was.  alpha = (float)(value / 1000.0).  With c_i = stft(istft(|S| angles_i)) the next phases are
 * those of t_i = c_i + alpha (c_i - c_{i-1}) (t_0 = c_0; a bin with t_i = 0 gets phase 0) -- librosa's and torchaudio's
 * `momentum`, whose rebuilt - momentum / (1 + momentum) * tprev is the same t up to a positive scale; the mse stays that of
 * the projection c_i of the last iteration.  It governs tts_griffin_lim, tts_synthesize and tts_synthesize_host alike.  With
 * alpha > 0 the previous projection is kept per bin in float32 (8 B x B x T x 1056 of workspace at n_fft 2048, allocated
 * by the first such call) and every iteration is a launch of its own whatever "gl_pair" says; utterances stay independent
 * of each other, a call's waveform and mse are the same bits from run to run and whatever the cut into runs, and a NaN
 * magnitude makes its own utterance's waveform non-finite and its mse NaN and touches no other, all as for alpha = 0),
 * "gl_init" (how a Griffin-Lim call without an explicit `init_phase` starts: 0 (default) = random phases from `seed`,
 * 1 = phases estimated from the magnitudes the call reconstructs from, tts_phase_estimate below; any other value is
 * TTS_ERR_INVALID and leaves the option as it was.  With 1, a call of tts_griffin_lim, tts_griffin_lim_ragged, tts_synthesize
 * or tts_synthesize_host whose init_phase is NULL gives the bits of the same call with "gl_init" = 0 and init_phase =
 * tts_phase_estimate of its magnitudes -- in tts_synthesize those behind the speaking-rate / pitch stretch, at each
 * utterance's own frame count under end-of-speech stopping; `seed` is then unused, and in a pipelined call the estimate runs
 * on the main stream between the post-net (or the stretch) and the first Griffin-Lim launch.  An explicit init_phase always
 * wins.  With 0 nothing of a call changes),
 * "gl_wide_from" (pipelined calls: the first Griffin-Lim launch that is cut
 * for all compute units instead of all but "reserve_cus" -- the next call's decoder has left them by then; -1 (default) =
 * from a model of the two durations, -2 = never, n >= 0 = launch n; the waveform's bits do not depend on the cut),
 * "fused_tail" (default 1: lifter + highway stack + GRU input
 * projections of a CBHG as one launch; 0 = layer by layer), "enc_stream" (default 1: under the call pipeline with the
 * persistent decoder the encoder of a call runs on a stream of its own, one inter-Griffin-Lim gap ahead of its decoder, so
 * that the decoders of consecutive calls follow each other without a pause; tts_synthesize then waits on the HOST until the
 * device has reached the post-net of the call two back -- at most ~2.5 calls are ever queued; 0 = the encoder in front of
 * its decoder on the front stream, calls never block).
 * Test and diagnostic hooks -- per handle, inert (and refused with a non-zero value) until "debug_hooks" has been set to 1
 * on the same handle; nothing in the process environment changes what a call computes: "pd_debug_delay" (workgroup 3 of
 * every persistent-decoder cluster stages its tile that many x ~3.4 us late), "gl_runs" / "gl_run_len" (force the cut of
 * an utterance's frames into Griffin-Lim runs: runs per utterance / frames per run; the waveform's bits do not depend on
 * the cut), "gl_workers" (plan and launch Griffin-Lim for that many workgroups instead of one per free compute unit),
 * "pd_rows" (16 / 32: utterances per cluster of the weight-stationary decoder instead of the library's choice),
 * "timeline" (tts_profile_get prints the absolute times of every profiled span); tts_debug_hold.
 * Initial phases of Griffin-Lim: `init_phase` (a (B, F, T) array of U[0,1) numbers, angle = 2 pi u) or, when it is NULL,
 * a counter-based draw from `seed` made inside the first iteration's launch (the reference draws np.random.rand per call,
 * audio/synthesis.py:91). */
int tts_set_option(tts_handle_t h, const char* key, int value);
int tts_synchronize(tts_handle_t h);

/* Numerics: float32 throughout.  The dense and convolution layers form their f32 products from exact three-way bf16 splits of
 * both operands on the bf16 matrix pipe (same measured error against float64 as f32-input MFMA, tests/test_gpu_gemm.py).  One
 * difference from IEEE f32 arithmetic on non-finite values: an output that depends on a +-Inf operand is NaN (the split of Inf
 * contains Inf - Inf), not +-Inf; NaN operands give NaN; every output that depends on finite operands only is unaffected.
 * Non-finite values on the audio side: a NaN is never turned into a plausible finite number.  Where the reference clips
 * (np.clip, np.maximum: tts_denorm_power, the de-normalising epilogue of tts_synthesize's final Dense, tts_db_convert, the dB
 * and normalisation lines of tts_extract_features in features.hip) a NaN input gives a NaN output at the same element, as in
 * numpy, and +-Inf clip like any other value; every element that does not depend on the NaN keeps the bits of a clean run.
 * Where the reference takes a maximum (np.max: the loudest frame of tts_trim_bounds in features.hip) a NaN operand gives NaN.  A NaN magnitude makes the waveform of ITS utterance non-finite and its
 * Griffin-Lim mse NaN (the other utterances of the batch are untouched); no loop bound or wait of a kernel depends on data. */

/* ---- weights: replaces tf.train.Saver().restore (tacotron/inference.py:55,71) ---------- */
/* Manifest: names follow the TF variable scopes (see single-speaker-tts_amd/tacotron/weights.py). */
int tts_manifest_size(tts_handle_t h);
int tts_manifest_entry(tts_handle_t h, int index, const char** name, int64_t shape[4], int* ndim);
/* host_data: HOST pointer, TensorFlow layout (Dense (in,out); conv (k,in,out); GRU gates
 * (in+units, 2*units) = rows [input;state], columns [r|u]). */
int tts_set_weight(tts_handle_t h, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* All tensors of the manifest, concatenated in manifest order (the RCCL broadcast unit). */
int tts_load_weights_blob(tts_handle_t h, const float* host_blob, size_t n_floats);
/* Validates completeness, folds batch-norm, packs device layouts.  Synchronous. */
int tts_finalize_weights(tts_handle_t h);

/* ---- device memory helpers ---------------------------------------------------------- */
/* tts_malloc / tts_free act on the device that is CURRENT on the calling thread; with more than one GPU in
 * a process use the handle-bound pair, which allocates on the handle's device whatever is current. */
int tts_malloc(void** dptr, size_t bytes);
int tts_free(void* dptr);
int tts_device_malloc(tts_handle_t h, void** dptr, size_t bytes);
int tts_device_free(tts_handle_t h, void* dptr);
int tts_memcpy_h2d(tts_handle_t h, void* dst, const void* src, size_t bytes);  /* synchronous */
int tts_memcpy_d2h(tts_handle_t h, void* dst, const void* src, size_t bytes);  /* synchronous */
int tts_memset(tts_handle_t h, void* dst, int value, size_t bytes);

/* ---- network stages -------------------------------------------------------------------- */
/* Tacotron.encoder (tacotron/model.py:124-173): embedding + pre-net + CBHG.
 * ids int32 [B*Ts] -> memory float [B*Ts*2*n_gru_units].  An id outside [0, vocabulary_size) reads as
 * a zero embedding row (TensorFlow's GPU kernel does the same; its CPU kernel raises, which the Python
 * mirror reproduces for host arrays -- device-resident ids cannot be inspected without a sync). */
int tts_encoder_forward(tts_handle_t h, const int32_t* ids, int B, int Ts, float* memory);
/* Tacotron.decoder in Mode.PREDICT (tacotron/model.py:175-334; wrappers.py:94-124;
 * helpers.py:83-110,161-205): n_steps strictly sequential steps (reference: 1000//5 = 200).
 * memory [B*Ts*256] -> reduced mel [B * n_steps * (reduction*n_mels)] (== output_mel_spec
 * reshaped, model.py:383) and alignment_history [n_steps * B * Ts] (may be NULL). */
int tts_decoder_forward(tts_handle_t h, const float* memory, int B, int Ts, int n_steps,
                        float* mel, float* alignments);
/* Tacotron.post_process + final Dense (tacotron/model.py:336-363, 394-398).
 * mel [B*T*n_mels] -> output_linear_spec [B*T*(1+n_fft/2)]. */
int tts_postnet_forward(tts_handle_t h, const float* mel, int B, int T, float* linear);

/* ---- evaluation ------------------------------------------------------------------------- */
/* Tacotron in Mode.EVAL (tacotron/model.py:299-306, 432-442): encoder, free-running decoder for n_steps = T_red,
 * post-net + final Dense, then the three L1 losses against zero-padded targets.
 * mel_target [B * n_steps*r * n_mels], linear_target [B * n_steps*r * F] (device) ->
 * losses [3] = {loss, loss_decoder, loss_post_processing} (device, float);
 * optional (NULL to skip): l1_sums [B][2] (device, double), mel, alignments, linear as in tts_synthesize.
 * The stages are those of tts_encoder_forward / tts_decoder_forward (the stand-alone decoder choice,
 * tts_decoder_kernel_choice(h, B, Ts, 0)) / tts_postnet_forward: the spectrograms are theirs bit for bit.  The means
 * are float64 sums in a fixed order (per-utterance sums l1_sums[u] = {sum |mel_t - mel|, sum |lin_t - lin|}) rounded
 * once to float32, loss = loss_decoder + loss_post_processing in float32; the bits depend neither on the grid nor on
 * earlier calls.  NaN / Inf in a target or output give a NaN / Inf loss.  Float buffers must be 4-byte aligned. */
int tts_evaluate(tts_handle_t h, const int32_t* ids, int B, int Ts, int n_steps,
                 const float* mel_target, const float* linear_target, float* losses,
                 double* l1_sums, float* mel, float* alignments, float* linear);

/* ---- teacher forcing -------------------------------------------------------------------- */
/* The decoder fed as TacotronTrainingHelper feeds it (tacotron/helpers.py:208-405, chosen at tacotron/model.py:284-298):
 * the GO frame (zeros) at step 0 and frame t*r - 1 of the target at step t >= 1 (outputs[:, r-1::r]) instead of its own last
 * frame; the last r-frame group of the target is never fed.  Everything else is the inference network of Mode.PREDICT:
 * pre-net dropout off, batch norm from the moving statistics, no gradient -- this is NOT Mode.TRAIN.  Global and
 * LocalLuong attention (with tts_decoder_forward's refusals), both GRU formulations.
 * memory [B*Ts*256], mel_target [B * n_steps*r * n_mels] (device, 16-byte aligned; == (B, n_steps, r*n_mels)) ->
 * mel [B * n_steps * (r*n_mels)] and alignments [n_steps * B * Ts] (may be NULL), as tts_decoder_forward.
 * Decoder: tts_teacher_kernel_choice.  Given the padded shape (Ts, n_steps), an utterance's outputs depend neither on B,
 * on its position in the batch, on the rows per cluster nor on the calls the handle ran before.  Never graph-captured. */
int tts_decoder_forward_teacher(tts_handle_t h, const float* memory, int B, int Ts, int n_steps,
                                const float* mel_target, float* mel, float* alignments);
/* Teacher-forced forward pass of the whole network: tts_encoder_forward, tts_decoder_forward_teacher,
 * tts_postnet_forward (the post-net reads the teacher-forced mel prediction), then -- with linear_target != NULL --
 * the three L1 losses of tts_evaluate (tacotron/model.py:432-442, same kernels, same determinism and NaN rules):
 * losses [3] = {loss, loss_decoder, loss_post_processing}, optional l1_sums [B][2] (double).  linear_target == NULL:
 * no losses (losses, l1_sums ignored).  mel, alignments, linear: optional outputs (NULL to skip) as in tts_evaluate.
 * Arguments are checked as tts_evaluate checks them; mel_target must be 16-byte aligned. */
int tts_teacher_forced(tts_handle_t h, const int32_t* ids, int B, int Ts, int n_steps,
                       const float* mel_target, const float* linear_target, float* losses,
                       double* l1_sums, float* mel, float* alignments, float* linear);
/* Which decoder a teacher-forced call of this shape takes: 2 = the weight-stationary kernel's teacher variant
 * (decoder_ws.hip), where a stand-alone free-running call would take that kernel; 0 = launch per layer (decoder.hip) --
 * also where the free-running call would take decoder_persistent.hip (1), which has no teacher form.  Host only. */
int tts_teacher_kernel_choice(tts_handle_t h, int B, int T_sent);

/* ---- spectrogram de-normalisation ------------------------------------------------------ */
/* inference() post-step + synthesize() power (tacotron/inference.py:93-101,175;
 * audio/conversion.py:81-102, 32-53): per utterance transpose to (F,T),
 * db = (clip(x,0,1)-1)*(|ref|+|max|)+ref, mag = 10^(db/20), mag ** power.
 * linear [B*T*F] -> mag [B*F*T].  Returns TTS_ERR_DB_RANGE when some value de-normalises to less than
 * -100 dB (decibel_to_magnitude's assertion; checked on the data, and only for constants that allow it:
 * ref - |ref| - |max| < -100 -- the call then synchronises the stream).  A NaN in `linear` gives NaN at its transposed
 * position of `mag` and nothing else (np.clip and np.power carry it; it does not trip the -100 dB check), +Inf clips to 1
 * and -Inf to 0. */
int tts_denorm_power(tts_handle_t h, const float* linear, int B, int T, int F,
                     float ref_db, float max_db, float power, float* mag);

/* ---- Griffin-Lim ------------------------------------------------------------------------ */
/* griffin_lim_v2 / spectrogram_to_wav (audio/synthesis.py:5-125), batched.
 * mag [B*F*T] (F = 1+n_fft/2, reference layout (F,T) per utterance);
 * init_phase [B*F*T] of U[0,1) numbers = what np.random.rand returns at synthesis.py:85,
 * or NULL to draw them on device from `seed`;  wav [B * hop*(T-1)];  mse [B] or NULL
 * (mean squared magnitude error of the last iteration, synthesis.py:112). */
int tts_griffin_lim(tts_handle_t h, const float* mag, const float* init_phase, uint64_t seed,
                    int B, int T, int n_iter, int win_length, int hop_length, int n_fft,
                    float* wav, float* mse);
/* tts_griffin_lim for utterances of different lengths in one padded batch.  mag, init_phase: [B][F][T_max] as tts_griffin_lim
 * takes them; n_frames: HOST int32 [B], 1 <= n_frames[b] <= T_max with hop (n_frames[b] - 1) > n_fft / 2 for every b
 * (TTS_ERR_INVALID otherwise, naming the utterance, before anything is enqueued).  Columns t >= n_frames[b] of mag and
 * init_phase are never read.  wav [B][hop (T_max - 1)]: samples [0, hop (n_frames[b] - 1)) are
 * the reconstruction of utterance b alone -- the bits of tts_griffin_lim(B = 1, T = n_frames[b]) on its columns with the same
 * handle options, in the streaming and in the general kernels -- and the rest of its row is written as 0.  mse [B] or NULL: mean
 * over F x n_frames[b] (with "gl_momentum" and in the general kernels the bits of that single call, otherwise equal to rounding:
 * the plain streaming form sums per run).  init_phase == NULL draws bin (b, f, t) as tts_griffin_lim(B, T_max, seed) does.
 * n_frames[b] == T_max for every b gives the bits of tts_griffin_lim.  No model needs to be loaded. */
int tts_griffin_lim_ragged(tts_handle_t h, const float* mag, const float* init_phase, uint64_t seed, int B, int T_max,
                           const int32_t* n_frames, int n_iter, int win_length, int hop_length, int n_fft,
                           float* wav, float* mse);
/* librosa.output.write_wav(norm=True) scaling (audio/io.py:53): wav /= max|wav| per
 * utterance unless the peak is below FLT_MIN.  In place, wav [B*n].  NaN samples stay NaN and do not take part in the peak
 * search (numpy's max would make the whole utterance NaN): the finite samples of that utterance are scaled by the peak of
 * the finite ones, other utterances are not affected. */
int tts_peak_normalize(tts_handle_t h, float* wav, int B, int n);

/* ---- end of speech ---------------------------------------------------------------------- */
/* silence_interval_from_spectrogram (audio/effects.py:218-233; the criterion of the TODO at tacotron/inference.py:76-78,
 * which the reference never calls), batched, and the frame count that follows from it.
 * spec: DEVICE [B][T][row_stride], time-major; the first F floats of a row are its data, columns F .. row_stride - 1 are never
 * read (tts_postnet_forward's `linear` has row_stride == F; the magnitude rows of tts_synthesize are padded).  Frame t of
 * utterance b is ACTIVE iff np.max(row) > threshold as numpy evaluates it: the comparison is strict, a row that holds a NaN
 * anywhere is silent (np.max carries the NaN, the comparison is False), +Inf is active, a row of -Inf is silent.
 *   last_active[b] = the largest active t, -1 when there is none (the reference's trim_end / None); DEVICE int32 [B] or NULL
 *   n_frames[b]    = min(T, max(min_frames, last_active[b] + 1 + keep_frames));                    DEVICE int32 [B]
 * The threshold is in the units of the buffer (tts_speech_threshold converts decibels); nothing is computed on the data, so
 * the result is exact and the same whatever B and the utterance's place in the batch.  Two launches, asynchronous, no model
 * needed.  TTS_ERR_INVALID, before anything is enqueued: B, T, F < 1, row_stride < F, keep_frames < 0, min_frames outside
 * [1, T], a NaN threshold, a NULL spec or n_frames. */
int tts_speech_frames(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride,
                      float threshold, int keep_frames, int min_frames,
                      int32_t* n_frames, int32_t* last_active /* may be NULL */);
/* A threshold in decibels in the units of a spectrogram buffer, computed in double and rounded once to float.
 * units TTS_SPEECH_NORMALIZED_DB: the network's `linear`, x = (threshold_db - ref_db) / (|ref_db| + |max_db|) + 1 (the inverse
 * of inv_normalize_decibel, audio/conversion.py:81-102; `power` ignored); TTS_SPEECH_MAGNITUDE_POWER: the de-normalised
 * magnitudes ** power, m = pow(pow(10, threshold_db / 20), power) (ref_db, max_db ignored).  Both maps are monotone: the
 * comparison in either domain is the reference's comparison in dB up to the float32 rounding of the data.  Host only.
 * TTS_ERR_INVALID: a NaN argument that is used, |ref_db| + |max_db| == 0, power <= 0, unknown units, NULL out. */
#define TTS_SPEECH_NORMALIZED_DB 0
#define TTS_SPEECH_MAGNITUDE_POWER 1
int tts_speech_threshold(float threshold_db, float ref_db, float max_db, float power, int units, float* out);
/* Both ends of silence_interval_from_spectrogram (audio/effects.py:218-232 returns (trim_start, trim_end); tts_speech_frames
 * takes the end alone).  spec, row_stride, the activity rule and its NaN / Inf rules as tts_speech_frames has them:
 *   first_active[b] = the smallest active t, last_active[b] = the largest; both -1 when utterance b has no active frame (the
 *                     reference's None).  DEVICE int32 [B] each; last_active is what tts_speech_frames reports.
 * Exact, and the same whatever B and the utterance's place in the batch.  Two launches (the rows, then the utterances),
 * asynchronous, no model needed; profile stage "speech_end".  TTS_ERR_INVALID, before anything is enqueued: B, T, F < 1,
 * row_stride < F, a NaN threshold, a NULL spec, first_active or last_active. */
int tts_speech_interval(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold,
                        int32_t* first_active, int32_t* last_active);

/* ---- speaking rate ---------------------------------------------------------------------- */
/* time_stretch (audio/effects.py:46-88) as far as it reaches Griffin-Lim: the reference runs librosa 0.6 phase_vocoder(stft, rate)
 * and keeps np.abs of the result, and |mag exp(1j phase)| = mag -- what is left of the vocoder is a linear blend of neighbouring
 * magnitude frames.  For one utterance of n frames x[:, 0 .. n - 1] and a rate r (> 1 faster, < 1 slower):
 *   n_out   = ceil(n / r), the division and the ceil in double = len(np.arange(0, n, r, dtype=float))
 *   s = k r, i = (int)s, a = s - floor(s);   y[:, k] = (float)((1 - a) x[:, i] + a x[:, i + 1])          for k < n_out
 * in double, every operation rounded on its own (no FMA) and the result rounded once to float32; columns i >= n are the vocoder's
 * zero padding: they read as 0.0 and are never fetched.  The blend is always evaluated: 0 * NaN and 0 * Inf stay NaN as in numpy,
 * a NaN is never turned into a finite number, and every element that does not depend on it keeps the bits of a clean run.
 * Against the reference's whole path (phases carried, complex64, np.abs) the result differs by at most 2^-22 relative. */
/* Host only: *out = n_out above.  TTS_ERR_INVALID: n_frames < 1, a rate that is not finite or outside [0.25, 4], NULL out. */
int tts_stretched_frames(int n_frames, double rate, int* out);
/* The blend on magnitudes in the reference layout, as tts_griffin_lim and tts_stft_magnitude hold them: mag [B][F][T] ->
 * out [B][F][T_out].  n_frames: HOST int32 [B], the frames of each utterance, or NULL (all T); columns t >= n_frames[b] of mag are
 * never read.  Row b of out holds stretched_frames(n_frames[b]) blended frames and 0 from there to T_out.  64-bit indexing, no
 * atomics: an utterance's output is the same bits whatever B is and wherever it sits in the batch.  rate 1.0 is legal and returns
 * the input bits for finite data.  One launch per 64 utterances, asynchronous (the lengths travel in the launch: nothing is
 * uploaded), no model needed; profile stage "stretch".  TTS_ERR_INVALID, before anything is enqueued: a rate that is not finite
 * or outside [0.25, 4], B, F or T < 1, an n_frames[b] outside [1, T], T_out smaller than the largest stretched length, a NULL
 * mag or out. */
int tts_stretch_magnitudes(tts_handle_t h, const float* mag, int B, int F, int T, const int32_t* n_frames, double rate, int T_out,
                           float* out);
/* The same arithmetic (the same bits for the same values) on time-major padded rows, the layout of tts_speech_frames and of the
 * call pipeline: spec [B][T][row_stride] -> out [B][T_out][row_stride], the first F floats of a row are its data, columns
 * F .. row_stride - 1 are neither read nor written.  Rows t >= n_frames[b] of spec are never read.  With row_stride % 4 == 0 and
 * both buffers 16-byte aligned the rows move in 16-byte accesses.  Arguments and refusals as tts_stretch_magnitudes, and
 * row_stride < F. */
int tts_stretch_rows(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, const int32_t* n_frames, double rate,
                     int T_out, float* out);

/* ---- estimated initial phases ----------------------------------------------------------- */
/* A start for Griffin-Lim from the magnitudes alone: one pass that tracks spectral peaks from frame to frame (after Beauregard,
 * Harish and Wyse, "Single pass spectrogram inversion", 2015), in the format of `init_phase`.  The reference starts from
 * np.random.rand (audio/synthesis.py:85); from this estimate the loop reaches the mse of 60 iterations in about 12.
 * Phases are turns in unsigned 32-bit fixed point (angle = 2 pi phi / 2^32, additions wrap), phi_{-1}[k] = 0.  For frame t of
 * an utterance with m = mag[:, t], F = 1 + n_fft / 2, every comparison on the float32 values:
 *   bin j, 1 <= j <= F - 2, is a peak if m[j] > m[j-1] and m[j] > m[j+1].  With a, b, g = m[j-1], m[j], m[j+1] as doubles,
 *     p = 0.5 * (a - g) / ((a - 2.0 * b) + g);  x = ((double)hop_length * ((double)j + p)) / (double)n_fft;  fr = x - floor(x)
 *     adv = (uint32)floor(fr * 4294967296.0)   (every operation rounded on its own, no FMA; 0 where fr is not finite)
 *     phi_t[j] = phi_{t-1}[j] + adv
 *   a bin k that is no peak walks right while m[i] < m[i+1]; if the walk ends at a peak j, j owns k.  Otherwise it walks left
 *     while m[i] < m[i-1], likewise.  A walk that ends at a tie or at an edge finds no owner; comparisons with NaN are false,
 *     so a NaN bin is no peak and ends every walk.  An owned bin takes phi_t[k] = phi_t[j] + ((k - j) & 1) * 0x80000000 (the
 *     centred, unrotated frames of librosa's stft carry (-1)^k across a lobe); any other bin keeps phi_{t-1}[k].
 *   init_phase_out[b][k][t] = (float)(phi_t[k] >> 8) * 2^-24: exact, in [0, 1).
 * Everything but adv is integer arithmetic, so the result is the same bits whatever B is, wherever an utterance sits in the batch
 * and however the library cuts the frames (chunks of tts_phase_chunk_frames() frames whose maps are composed, chained and
 * applied); tests/phase_oracle.py restates the definition sequentially.
 * mag [B][F][T] as tts_griffin_lim takes it -> init_phase_out [B][F][T].  n_frames: HOST int32 [B], the frames of each utterance,
 * or NULL (all T); columns t >= n_frames[b] of mag are never read and those of init_phase_out never written.  Asynchronous on the
 * handle's stream (the lengths travel in the launches), no atomics, no loop bound or wait that depends on the data, no model
 * needed; profile stage "phase_init".  TTS_ERR_INVALID, before anything is enqueued: a NULL mag or init_phase_out, an n_fft that
 * is no power of two in 256 .. 4096, hop_length outside 1 .. n_fft, B or T < 1, T > 2^22, an n_frames[b] outside [1, T]. */
int tts_phase_estimate(tts_handle_t h, const float* mag, int B, int T, const int32_t* n_frames /* may be NULL */, int n_fft,
                       int hop_length, float* init_phase_out);
/* The same estimate (the same bits for the same values) from time-major padded rows, the layout of tts_speech_frames and of the
 * call pipeline -- what Griffin-Lim itself reads: spec [B][T][row_stride], the first 1 + n_fft / 2 floats of a row are its data,
 * the rest and rows t >= n_frames[b] are never read.  init_phase_out is the public [B][F][T] array all the same.  Arguments and
 * refusals as tts_phase_estimate, and row_stride < 1 + n_fft / 2. */
int tts_phase_estimate_rows(tts_handle_t h, const float* spec, int B, int T, int row_stride, const int32_t* n_frames, int n_fft,
                            int hop_length, float* init_phase_out);
/* Host only: the frames of one chunk of the estimate's cut in time (the results do not depend on it; tests place their shapes
 * around it). */
int tts_phase_chunk_frames(void);

/* ---- resampling ------------------------------------------------------------------------- */
/* librosa 0.6 resample(..., res_type='kaiser_best') = resampy 0.2 resample_f with the 'kaiser_best' windowed sinc: the second half
 * of pitch_shift (audio/effects.py:9-43) and what load_wav(sampling_rate=...) runs.  The filter is regenerated from resampy's
 * published design (num_zeros 64, 512 table samples per zero crossing, Kaiser beta 14.769656459379492, rolloff
 * 0.9475937167399596): win[j] = kaiser(2 n + 1, beta)[n + j] rolloff sinc(rolloff j / 512), j = 0 .. n = 32768, times rho for a
 * ratio rho = target rate / source rate < 1; delta[j] = win[j + 1] - win[j], delta[n] = 0.  With scale = min(1, rho),
 * step = (int)(512 scale) (resampy's truncation, kept) and inc = 1 / rho, output sample t of an utterance of n_in samples is
 *   tr = t inc, m = (int)tr, frac = scale (tr - m);   f = 512 frac, off = (int)f, eta = f - off
 *   y  = sum_i (win[off + i step] + eta delta[off + i step]) x[m - i]          i < min(m + 1, (32769 - off) / step)
 *      + the same with frac = scale - frac on x[m + 1 + k]                      k < min(n_in - m - 1, (32769 - off) / step)
 * the position in double, every operation rounded on its own; weights, products and sums in double, rounded once to float32.
 * resampy writes (long long)(n_in rho) samples and librosa zero-pads them to ceil(n_in rho). */
/* Host only: *out = ceil(n * ratio).  TTS_ERR_INVALID: n < 1, a ratio that is not finite or outside [0.25, 4], NULL out. */
int tts_resampled_length(int n, double ratio, int* out);
/* wav [B][n] -> out [B][N_out].  n_samples: HOST int32 [B], the samples of each utterance, or NULL (all n); samples at or behind
 * n_samples[b] are never read.  Row b of out holds min((long long)(n_samples[b] ratio), N_out) computed samples and 0.0 from
 * there to N_out (librosa's fix_length, in both directions).  A NaN or Inf input sample reaches every output whose window covers
 * it and no other.  64-bit indexing, no atomics: an utterance's output is the same bits whatever B is and wherever it sits in
 * the batch.  ratio 1.0 is legal and runs the filter.  Asynchronous on the handle's stream (the lengths travel in the launches;
 * the first call at a ratio builds that ratio's table on the host and uploads it with a synchronous copy, which blocks the
 * calling thread; ratios of 1 and above share one table), no model needed; profile stage "resample".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL wav or out, a ratio that is not finite or outside [0.25, 4], B, n or
 * N_out < 1, an n_samples[b] outside [1, n]. */
int tts_resample(tts_handle_t h, const float* wav, int B, int n, const int32_t* n_samples, double ratio, int N_out, float* out);

/* ---- analysis features (audio/features.py:5-86,116-145) and dB helpers ---------------- */
/* librosa.stft(wav, n_fft, hop, win) as linear_scale_spectrogram returns it (features.py:145):
 * centre/reflect padding, periodic hann.  wav [B*n] -> out complex64 interleaved
 * [B*F*n_frames*2], n_frames = 1 + n/hop. */
int tts_stft(tts_handle_t h, const float* wav, int B, int n, int n_fft, int win_length,
             int hop_length, float* out);
/* abs(stft) ** power (features.py:62-71).  wav [B*n] -> lin [B*F*n_frames]. */
int tts_stft_magnitude(tts_handle_t h, const float* wav, int B, int n, int n_fft, int win_length,
                       int hop_length, float power, float* lin);
/* np.dot(librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=True), lin) (features.py:75-84).
 * lin [B*F*n_frames] -> mel [B*n_mels*n_frames]. */
int tts_mel_spectrogram(tts_handle_t h, const float* lin, int B, int n_frames, int n_fft,
                        int sampling_rate, int n_mels, float fmin, float fmax, float* mel);
/* Elementwise audio/conversion.py: mode 0 magnitude_to_decibel (:5-29), 1 decibel_to_magnitude
 * (:32-53; TTS_ERR_DB_RANGE if any input < -100, synchronous), 2 normalize_decibel (:56-78),
 * 3 inv_normalize_decibel (:81-102).  in/out [n] (may alias).  NaN in gives NaN out in every mode (np.maximum(1e-5, nan)
 * and np.clip(nan, 0, 1) are NaN; a NaN does not trip mode 1's range check); +-Inf clip like any other value. */
int tts_db_convert(tts_handle_t h, const float* in, size_t n, int mode, float ref_db, float max_db,
                   float* out);

/* ---- dataset features (reference datasets/lj_speech.py:106-156 load_audio, dataset_helper.py:326-356) ------------ */
/* A RAGGED batch of B recordings: samples back to back in `wav` (device, float32), recording b is
 * wav[offsets[b] .. offsets[b+1]) with `offsets` a HOST array of B + 1 non-decreasing int64 (offsets[0] = 0 is not required).
 *
 * librosa.effects.trim (librosa 0.6) of every recording: reflect padding by frame_length / 2, frames k = 0 .. n / hop,
 * mse_k = mean square of the frame (float64), frame k non-silent iff 10 log10(max(1e-10, mse_k)) - 10 log10(max(1e-10,
 * max mse)) > -top_db (float64), bounds[2b] = first * hop, bounds[2b + 1] = min(n, (last + 1) * hop).  bounds: DEVICE int64
 * [2B].  Needs n > frame_length / 2 for every recording (TTS_ERR_INVALID otherwise) and top_db > 0.  Two launches whatever
 * B and the lengths are; asynchronous.
 * Non-finite samples are decided as numpy decides them: a NaN anywhere in a recording makes the maximum, and with it the
 * reference level, NaN, every comparison is false, no frame is non-silent and the bounds are {0, 0}; a +-Inf sample gives
 * {0, 0} too (Inf - Inf in its frames, -Inf in the others).  The other recordings of the batch are untouched. */
int tts_trim_bounds(tts_handle_t h, const float* wav, const int64_t* offsets, int B, int frame_length, int hop_length,
                    float top_db, int64_t* bounds);

/* The feature pass.  ALWAYS start from tts_default_feature_params (fills `struct_size` and the model's values). */
typedef struct tts_feature_params {
    int32_t struct_size;         /* sizeof(tts_feature_params_t) of the caller's header */
    int32_t n_fft;               /* 2048: a power of two, 256 .. 4096 */
    int32_t win_length;          /* 1102: 2 .. n_fft */
    int32_t hop_length;          /* 275 */
    int32_t sampling_rate;       /* 22050 */
    int32_t n_mels;              /* 80 (HTK mel filterbank, norm 1, librosa 0.6) */
    float fmin, fmax;            /* 0, 8000 (fmax <= 0: sampling_rate / 2) */
    float mel_ref_db, mel_max_db;        /* 6.02, 99.89 (LJSpeechDatasetHelper) */
    float linear_ref_db, linear_max_db;  /* 35.66, 100 */
    int32_t normalize;           /* 1: normalize_decibel of both rows; 0: raw dB (magnitude_to_decibel) */
    int32_t reduction;           /* 5: frames are zero-padded to a multiple of it */
    int32_t trim;                /* 1: features of the trimmed segment (tts_trim_bounds); 0: of the whole recording */
    float trim_top_db;           /* 60 */
    int32_t trim_frame_length;   /* 2048 */
    int32_t trim_hop_length;     /* 512 */
} tts_feature_params_t;
int tts_default_feature_params(tts_feature_params_t* p);
/* Planning: plan (HOST int64 [3B]) = {start, end, T_pad} per recording -- the analysed segment wav[offsets[b] + start ..
 * offsets[b] + end) (the trim bounds, or the whole recording) and its frame count 1 + (end - start) / hop zero-padded to a
 * multiple of p->reduction.  With p->trim this enqueues tts_trim_bounds and synchronises the stream once to read the bounds
 * back; without, nothing is enqueued.  A segment of at most n_fft / 2 samples is refused with TTS_ERR_INVALID (reflect
 * padding is undefined there). */
int tts_plan_features(tts_handle_t h, const float* wav, const int64_t* offsets, int B, const tts_feature_params_t* p,
                      int64_t* plan);
/* For every recording and frame t < T_pad of its plan: |STFT| of the segment (periodic hann, centred, reflect padding by
 * n_fft / 2 about the SEGMENT's ends), then the rows
 *   lin[t] = normalize_decibel(magnitude_to_decibel(|X_t|), linear_ref_db, linear_max_db)    (F = 1 + n_fft / 2 values)
 *   mel[t] = normalize_decibel(magnitude_to_decibel(M |X_t|), mel_ref_db, mel_max_db)       (n_mels values)
 * (raw dB when p->normalize is 0), and 0 in the padding rows t >= 1 + (end - start) / hop.  Outputs (device, float32) are
 * time-major and ragged: recording b's rows follow those of recording b - 1, mel_out [sum T_pad][n_mels], lin_out
 * [sum T_pad][F] -- per recording the reference's (T_pad / r, n_mels r) / (T_pad / r, F r) arrays.  One launch; a recording's
 * rows are the same bits whatever batch it is in and at whatever position.  Asynchronous; the plan is read on the host.
 * Non-finite samples: a NaN sample makes every linear value NaN, and every mel value whose band is not empty, in exactly the
 * frames whose win_length span holds it, raw or normalised (np.maximum(1e-5, nan) and np.clip(nan, 0, 1) are NaN: it never
 * comes out as -100 dB or 0.0); a +-Inf sample gives NaN or the image of +Inf (inf raw, 1.0 normalised) there.  Every other
 * frame and recording keeps the bits of a clean run.  With p->trim, tts_plan_features refuses a recording that holds a
 * non-finite sample: its trim bounds are {0, 0}, "at most n_fft / 2" samples. */
int tts_extract_features(tts_handle_t h, const float* wav, const int64_t* offsets, int B, const tts_feature_params_t* p,
                         const int64_t* plan, float* mel_out, float* lin_out);

/* ---- cepstra and alignment: mel-cepstral distortion --------------------------------------- */
/* calculate_mfccs (audio/features.py:89-113): librosa.feature.mfcc(S=mel_spec, n_mfcc=n) with S given is the orthonormal DCT-II of
 * S along the mel axis, first n rows, with no dB conversion of its own.  On time-major rows, the layout of the network's mel output
 * and of the dataset features: spec DEVICE [B][T][row_stride] -> out DEVICE [B][T][n_mfcc],
 *   out[b][t][k] = (float) sum_{n = 0 .. n_mels - 1} d[k][n] x[n]
 *   d[k][n] = sqrt(2 / n_mels) cos(pi k (2 n + 1) / (2 n_mels)), row 0 times 1 / sqrt(2), built on the host in double
 *   x[n] = (double)spec[b][t][n], or with clip01 != 0 np.clip(spec, 0, 1) of it as numpy clips (a NaN stays NaN; the reference
 *          clips the network's output before it de-normalises it, tacotron/inference.py:93-101)
 * products and the sum in double, n ascending, the result rounded once to float32: against a float64 evaluation y of the same sum
 * |out - y| <= 2^-24 |y| + 2^-40 sum_n |d[k][n]| |x[n]|.  n_frames: HOST int32 [B], the frames of each utterance, or NULL (all T);
 * rows t >= n_frames[b] are never read and are written as 0; columns n_mels .. row_stride - 1 are never read.  A NaN input makes
 * its own frame's coefficients NaN and touches nothing else.  No model needed, no atomics; asynchronous on the handle's stream
 * (the lengths travel in the launch; the first call at a pair (n_mels, n_mfcc) builds that table on the host and uploads it with
 * a synchronous copy); one launch per 64 utterances; profile stage "mfcc".  TTS_ERR_INVALID, before anything is enqueued: a
 * NULL spec or out, B, T, n_mels or n_mfcc < 1, n_mels > 1024, n_mfcc > n_mels, row_stride < n_mels, an n_frames[b] outside
 * [1, T]. */
int tts_mfcc(tts_handle_t h, const float* spec, int B, int T, int n_mels, int row_stride,
             const int32_t* n_frames /* HOST [B] or NULL */, int n_mfcc, int clip01, float* out /* [B][T][n_mfcc] */);
/* Dynamic time warping of B pairs of feature sequences (no reference counterpart: the alignment under which audio/metrics.py
 * measures mel-cepstral distortion).  a DEVICE [B][Ta][stride_a], b DEVICE [B][Tb][stride_b]: the first D floats of a row are the
 * frame, the rest is never read (a caller skips c0 by passing ptr + 1, D = K, stride = K + 1).  n_a / n_b: HOST int32 [B], the
 * frames of each sequence, or NULL (all Ta / Tb); frames at or behind them are never read.  For one pair with na and nb frames:
 *   local cost   c(i, j) = sqrt(s) with s = 0.0; for d in 0 .. D - 1: t = (double)a[i][d] - (double)b[j][d]; s = s + t * t
 *                every operation an IEEE double operation rounded on its own (no FMA), sqrt correctly rounded
 *   first cell   Dm(0, 0) = c(0, 0), L(0, 0) = 1
 *   other cells  candidates in the order diagonal (i - 1, j - 1), up (i - 1, j), left (i, j - 1), those inside the table only;
 *                best = the first that exists, a later one replaces it iff its Dm is strictly smaller;
 *                Dm(i, j) = c(i, j) + Dm(best), L(i, j) = L(best) + 1
 *   cost[p] = Dm(na - 1, nb - 1) (DEVICE double [B]), path_len[p] = L(na - 1, nb - 1) (DEVICE int32 [B])
 *   path[p][k] = (i_k, j_k), k < path_len[p]: the chain of `best` choices from (0, 0) to (na - 1, nb - 1) in forward order; rows
 *                k >= path_len[p] are written as (-1, -1).  DEVICE int32 [B][Ta + Tb - 1][2], or NULL.
 * Exactness: every operation is an individually rounded double operation or an integer one, so cost is the bits of the sequential
 * evaluation (tests/dtw_oracle.py) and path_len and path are integer-equal to it, whatever order the library walks the table in
 * (anti-diagonals, cut into pieces of tts_dtw_tile() cells).  Independence: a pair's results do not depend on B, on its place in
 * the batch, on Ta / Tb or on earlier calls.  NaN: comparisons with NaN are false, so a NaN anywhere in the first D floats of a
 * frame < na / < nb makes that pair's cost NaN (every monotone path crosses every row and column); its path_len and path are
 * still what the rule gives, and the other pairs keep the bits of a clean run.  Inf follows IEEE arithmetic.  No loop bound or
 * wait depends on the data: the table is walked in na + nb - 1 diagonals and the path in at most na + nb - 1 steps, both from
 * the host lengths, which travel in the launch.  No atomics.  No model needed; asynchronous on the handle's stream, one launch
 * per 64 pairs; profile stage "dtw".  With a path the call keeps 2 bits per cell in workspace of the handle, which grows as the
 * other workspaces do (a call that needs more than any before synchronises the handle).
 * Limits: 1 <= D <= 128 and na, nb <= tts_dtw_max_frames() (2048: 25 s at a hop of 275 samples of 22050 Hz); beyond them
 * TTS_ERR_UNSUPPORTED, and the message names the limit.  TTS_ERR_INVALID, before anything is enqueued: a NULL a, b, cost or
 * path_len, B, Ta, Tb or D < 1, a stride < D, a length outside [1, Ta] / [1, Tb], a cost that is not 8-byte aligned. */
int tts_dtw(tts_handle_t h, const float* a, int Ta, int stride_a, const int32_t* n_a /* HOST [B] or NULL */,
            const float* b, int Tb, int stride_b, const int32_t* n_b /* HOST [B] or NULL */,
            int B, int D, double* cost /* [B] */, int32_t* path_len /* [B] */,
            int32_t* path /* [B][Ta + Tb - 1][2] or NULL */);
/* Host only: the longest sequence tts_dtw takes. */
int tts_dtw_max_frames(void);
/* Host only: the cells of one piece of the cut of an anti-diagonal (no result depends on it; tests place their shapes around it). */
int tts_dtw_tile(void);

/* ---- F0 tracking: F0 RMSE, voicing error and gross pitch error ------------------------------ */
/* The fundamental frequency of B waveforms by YIN (de Cheveigne and Kawahara 2002, steps 2 to 5; no reference counterpart: the
 * track under which audio/metrics.py measures F0 RMSE, voicing error and gross pitch error).  wav DEVICE [B][N]; n_samples: HOST
 * int32 [B], the samples of each utterance, or NULL (all N).  T = tts_f0_frames(N, hop) = 1 + N / hop values per row; utterance b
 * has T_b = tts_f0_frames(n_b, hop) frames, frame t at sample t * hop -- the frames of the centred STFT: a hop (T - 1)-sample
 * Griffin-Lim waveform gives T values.  x(i) = (double)wav[b][i] for 0 <= i < n_b and 0.0 otherwise; samples at or behind n_b are
 * never read.  For frame t, with s0 = t * hop - (W + tau_max) / 2 (integer division):
 *   difference     for tau in 1 .. tau_max: s = 0.0; for j in 0 .. W - 1: u = x(s0 + j) - x(s0 + j + tau); s = s + u * u; d[tau] = s
 *                  every operation an IEEE double operation rounded on its own (no FMA)
 *   normalisation  c = 0.0; for tau ascending: c = c + d[tau]; q[tau] = (c == 0.0) ? 1.0 : (d[tau] * (double)tau) / c
 *   non-finite     a final c that is not finite (a NaN or Inf sample in the span): f0 and aperiodicity of the frame are NaN, and
 *                  nothing below applies; no other frame and no other utterance is touched
 *   threshold      tau1 = the smallest tau in [tau_min, tau_max] with q[tau] < threshold.  None: the frame is unvoiced, f0 = 0 and
 *                  aperiodicity = (float)q[best], best = the first index of the minimum over [tau_min, tau_max] (a later value
 *                  replaces it only if strictly smaller)
 *   descent        tau* = the smallest tau >= tau1 with tau == tau_max or not q[tau + 1] < q[tau]
 *   interpolation  delta = 0.0; if tau* < tau_max: a = q[tau* - 1], b = q[tau*], g = q[tau* + 1], den = (a + g) - (b + b), and
 *                  if a >= b && g >= b && den > 0: delta = (0.5 * (a - g)) / den
 *   f0[b][t] = (float)(sampling_rate / ((double)tau* + delta)), aperiodicity[b][t] = (float)q[tau*]
 *   padding        frames t >= T_b are written as 0
 * f0 DEVICE float [B][T]; aperiodicity DEVICE float [B][T] or NULL.  Exactness: f0 and aperiodicity are the bits of the sequential
 * evaluation (tests/f0_oracle.py) whatever the library's cut into lags, frames and workgroups.  Independence: an utterance's
 * results do not depend on B, on its place in the batch, on N or on earlier calls.  No loop bound or wait depends on the data;
 * no atomics.  No model needed; asynchronous on the handle's stream, one launch per 64 utterances (the lengths travel in the
 * launch); profile stage "f0".
 * Limits: 1 <= W <= tts_f0_max_window() (2048) and 2 <= tau_min <= tau_max <= tts_f0_max_lag() (1024: 21.5 Hz at 22050 Hz); beyond
 * them TTS_ERR_UNSUPPORTED, and the message names the limit.  TTS_ERR_INVALID, before anything is enqueued: a NULL wav or f0, B,
 * N or hop < 1, a length outside [1, N], a sampling_rate that is not finite and positive, a NaN threshold. */
int tts_f0(tts_handle_t h, const float* wav /* [B][N] */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
           double sampling_rate, int hop, int W, int tau_min, int tau_max, double threshold,
           float* f0 /* [B][T] */, float* aperiodicity /* [B][T] or NULL */);
/* Host only: the values tts_f0 writes for n samples, 1 + n / hop (0 for n < 0 or hop < 1). */
int tts_f0_frames(int n, int hop);
/* Host only: the largest W and the largest tau_max tts_f0 takes. */
int tts_f0_max_window(void);
int tts_f0_max_lag(void);
/* The F0 and voicing errors of B pairs of tracks along alignment paths.  f0_a DEVICE [B][Ta], f0_b DEVICE [B][Tb] (side b is the
 * recording); path DEVICE int32 [B][rows][2] as tts_dtw writes it: all `rows` rows are walked, and rows with a negative entry
 * (those behind the path), or an entry at or beyond Ta / Tb, are skipped.  For every step (i, j) in row order, with
 * fa = (double)f0_a[i], fb = (double)f0_b[j]; voiced means > 0:
 *   counts[0] every step;  counts[4] a step with a NaN on either side, which counts nowhere else
 *   counts[2] exactly one side voiced
 *   both voiced: counts[1]; u = fa - fb, sums[0] = sums[0] + u * u (a product and a sum, in row order: the bits of
 *                tests/f0_oracle.py); counts[3] when fabs(u) > 0.2 * fb (gross pitch error, 20 %);
 *                z = 1200.0 * log2(fa / fb), sums[1] = sums[1] + z * z (through the device's log2: against a float64 evaluation
 *                S64, |sums[1] - S64| <= 2e-12 sum |z_k| + 1e-15 S64)
 * counts DEVICE int32 [B][5], sums DEVICE double [B][2] (8-byte aligned).  No atomics, the loop bound is `rows`; one launch,
 * asynchronous on the handle's stream; profile stage "f0".  TTS_ERR_INVALID, before anything is enqueued: a NULL pointer, B, Ta,
 * Tb or rows < 1, sums not 8-byte aligned. */
int tts_f0_compare(tts_handle_t h, const float* f0_a, int Ta, const float* f0_b, int Tb, const int32_t* path /* [B][rows][2] */,
                   int rows, int B, int32_t* counts /* [B][5] */, double* sums /* [B][2] */);

/* ---- intelligibility: STOI and ESTOI ------------------------------------------------------- */
/* Short-time objective intelligibility (Taal, Hendriks, Heusdens and Jensen 2011) and its extended form (Jensen and Taal 2016)
 * of B pairs of time-aligned mono waveforms at 10 000 Hz (no reference counterpart; resampling is the caller's job:
 * tts_resample).  ref, deg DEVICE [B][N]; n_samples: HOST int32 [B], the samples of each row, or NULL (all N) -- samples at or
 * behind n_samples[b] are never read.  Constants: frames of W = 256 samples, H = 128 apart, a transform of 512 points, J = 15
 * one-third octave bands from 150 Hz, segments of 30 frames, the clip constant c = 1 + 10 ** (15 / 20), a dynamic range of 1e-4
 * in energy (40 dB).  tts_stoi_window fills w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257) (np.hanning(258)[1:-1]) and tts_stoi_bands
 * the bins [lo, hi) of every band, lo and hi the bins nearest to 150 * 2 ** ((2 k -/+ 1) / 6) Hz: the host's cos / pow make the
 * tables once, and a restatement takes them from there.
 *
 * Per row with n samples, every operation an individually rounded IEEE double operation:
 *  1. frames = n < 256 ? 0 : (n - 256) / 128 + 1.
 *  2. E[m] = sum over i of t * t, t = w[i] * (double)ref[128 m + i]: E starts at 0.0 and takes the terms one by one in
 *     ascending i, E = E + t * t (a product and a sum), the same for every frame.
 *  3. Emax: the largest E[m] that is not NaN, or 0; frame m is kept iff E[m] > Emax * 1e-4.  kept: their count; kept_index: their
 *     indices idx[k], ascending.  These equal tests/stoi_oracle.py exactly.
 *  4. The compacted signals of (kept - 1) * 128 + 256 samples: xs[p] = the sum, in ascending k, of
 *     w[p - 128 k] * (double)ref[128 idx[k] + p - 128 k] over the at most two kept frames k that cover p; ys the same from deg.
 *  5. For m < kept: z[i] = w[i] * xs[128 m + i] zero-padded to 512 points, its DFT, P[k] = re^2 + im^2,
 *     X[j][m] = sqrt(sum of P[k] over lo_j <= k < hi_j) in ascending k; Y from ys.  With `envelopes` they are written for
 *     m < kept as [row][0: X, 1: Y][j][m], rows of cap = tts_stoi_frames(N) doubles; nothing else of the buffer is touched.
 *     Each signal has its own transform: a NaN in deg leaves X as it was, and a deg of zeros has Y == 0.0 exactly.
 *  6. segments = kept >= 30 ? kept - 29 : 0; segment s takes the frames s .. s + 29.
 *  7. extended = 0, per segment and band: a = ||x|| / ||y|| (sums of squares from 0.0 in frame order, sqrt, a quotient),
 *     y'_t = min(a y_t, c x_t) (a NaN on either side is a NaN), the means (a sum in frame order) / 30, and
 *     r = sum dx dy / (sqrt(sum dx dx) * sqrt(sum dy dy)) of the centred values.  A term with ||y|| == 0, sum dx dx == 0 or
 *     sum dy dy == 0 is 0 and counts in `degenerate`; there is no epsilon.  A segment's terms are added in band order from 0.0.
 *  8. extended = 1, per segment: every row of the 15 x 30 blocks of X and Y minus its mean, over its centred norm (a row of
 *     centred norm 0 becomes zeros and counts in `degenerate`), then every column of the result the same way (likewise), and
 *     d_s = (sum over columns t, then bands j, of xn * yn) / 30.
 *  9. value = (the segments' sums added in segment order from 0.0) / (15 * segments), extended: / segments.  segments == 0: NaN.
 *     A NaN in a kept sample of either signal makes value NaN; a reference frame that holds a NaN is not kept (the comparison
 *     is false); an Inf energy empties the row.
 * The order of every sum is fixed, so a row's record has the same bits alone, in any ragged batch, at any B and whatever the
 * handle ran before.  The envelopes and value are held to the bound of DESIGN.md against tests/stoi_oracle.py (the transform is
 * the device's own); from given envelopes, steps 6 to 9 are the oracle's bits.
 * records DEVICE [B] (8-byte aligned); kept_index DEVICE int32 [B][cap] or NULL; envelopes DEVICE double [B][2][15][cap] or NULL.
 * Five launches per 64 rows (the lengths travel by value), no host wait between them, no atomics, nothing uploaded but the
 * arguments; asynchronous on the handle's stream; profile stage "stoi".  TTS_ERR_INVALID, before anything is enqueued: a NULL
 * ref, deg or records, B or N < 1, an n_samples[b] outside 1 .. N, extended not 0 or 1, a misaligned buffer.
 * TTS_ERR_UNSUPPORTED: more than tts_stoi_max_frames() frames in N samples. */
typedef struct {
    int32_t frames, kept, segments, degenerate;
    double value;
} tts_stoi_record_t;                               /* 24 bytes */
int tts_stoi(tts_handle_t h, const float* ref /* [B][N] */, const float* deg /* [B][N] */, int B, int N,
             const int32_t* n_samples /* HOST [B] or NULL */, int extended, tts_stoi_record_t* records /* DEVICE [B] */,
             int32_t* kept_index /* DEVICE [B][cap] or NULL */, double* envelopes /* DEVICE [B][2][15][cap] or NULL */);
/* host only: the frames of n samples; the most frames tts_stoi takes; the window; the bands */
int tts_stoi_frames(int n);
int tts_stoi_max_frames(void);
int tts_stoi_window(double w[256]);
int tts_stoi_bands(int32_t edges[15][2]);

/* ---- loudness: ITU-R BS.1770-4 / EBU R 128 ------------------------------------------------ */
/* Integrated loudness of B mono utterances (no reference counterpart: the reference's only level control is the peak
 * normalisation of save_wav).  wav DEVICE [B][N]; n_samples: HOST int32 [B], the samples of each utterance, or NULL (all N) --
 * samples at or behind n_samples[b] are never read.  sampling_rate: an integer in 8000 .. 192000.  Every product, sum and
 * quotient below is an individually rounded IEEE double operation on x = (double)wav[b][i]:
 *   K-weighting    two biquads, b0 b1 b2 a1 a2 each (tts_loudness_filter: the bilinear transform, at this sampling rate, of the
 *                  analogue shelf and high-pass that give the standard's tables at 48 kHz), each in direct form II transposed:
 *                  y = b0 x + z1;  z1 = (b1 x - a1 y) + z2;  z2 = b2 x - a2 y
 *   the cut        s = sampling_rate / 10 samples are a step, K = n / s steps are read (none when K < 4), and the samples behind
 *                  them count for nothing.  A step is cut into 8 segments of c = tts_loudness_segment(sampling_rate) =
 *                  ceil(s / 8) samples, the last of s - 7 c.  Pass 1 runs the cascade over each segment from the zero state and
 *                  keeps the four state values e_i it ends in; pass 2 chains them, S_0 = 0 and
 *                  S_{i+1}[r] = ((((M[r][0] S_i[0] + M[r][1] S_i[1]) + M[r][2] S_i[2]) + M[r][3] S_i[3]) + e_i[r], where column j
 *                  of the segment's transition M is the state the same recurrence ends in from the unit state j on zero input;
 *                  pass 3 runs each segment again from S_i and sums y * y in sample order.  The cut depends on the sampling
 *                  rate alone (csrc/loudness_plan.h).
 *   blocks         u_k = the sum of step k's 8 segment sums in order; block j = steps j .. j + 3, J = K - 3 of them, with
 *                  z_j = (((u_j + u_j+1) + u_j+2) + u_j+3) / (4 s)
 *   gates          absolute: z_j > 1.1724653045822981e-07 (-70 LUFS); relative: also z_j > 0.1 * (the sum of the absolutely
 *                  gated z_j in block order / their count)
 *   mean_square[b] = the sum, in block order, of the z_j that pass both gates / their count; 0 when J < 1 or no block passes;
 *                  NaN when any z_j is not finite (a NaN or Inf sample inside a counted block; one behind the last block
 *                  changes nothing).  LUFS = -0.691 + 10 log10(mean_square) is the host's to take.
 * mean_square DEVICE double [B]; n_blocks DEVICE int32 [B][2] or NULL: J, and the blocks that passed both gates (0 where
 * mean_square is NaN).  Exactness: the bits of tests/loudness_oracle.py.  Independence: an utterance's results are the bits of
 * the B = 1 call on its own samples.  No model needs to be loaded.  Asynchronous on the handle's stream (4 launches per 64
 * utterances); profile stage "loudness".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL wav or mean_square, B or N < 1, an n_samples[b] outside 1 .. N, a
 * misaligned buffer; TTS_ERR_UNSUPPORTED: a sampling rate outside 8000 .. 192000. */
int tts_loudness(tts_handle_t h, const float* wav /* [B][N] */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
                 int sampling_rate, double* mean_square /* [B] */, int32_t* n_blocks /* [B][2] or NULL */);
/* The same measurement, then a gain per utterance that takes it to target_lufs, in place:
 *   g = sqrt(Z_T / z), Z_T = 10 ** ((target_lufs + 0.691) / 10) taken on the host, z = mean_square[b];
 *   g = min(g, max_peak / peak), peak = the largest |x| among the finite samples of the utterance;
 *   g = 1 exactly where z is 0 or not finite, or peak is 0;
 *   wav[b][i] = (float)(g * (double)wav[b][i]) for i < n_samples[b] (a NaN sample stays NaN)
 * with a correctly rounded division and square root.  Samples at or behind n_samples[b] are neither read nor written.
 * mean_square DEVICE double [B] or NULL: as measured, before the gain; gain DEVICE double [B] or NULL.  Asynchronous on the
 * handle's stream; profile stage "loudness".  Refusals as tts_loudness (wav alone is required), and TTS_ERR_INVALID for a
 * target that is not finite or a max_peak that is not finite and positive. */
int tts_loudness_normalize(tts_handle_t h, float* wav /* [B][N], in place */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
                           int sampling_rate, double target_lufs, double max_peak, double* mean_square /* [B] or NULL */,
                           double* gain /* [B] or NULL */);
/* Host only, no handle and no device: b0 b1 b2 a1 a2 of the shelf, then of the high-pass, as the library designed them for this
 * sampling rate (tan and pow are the host libm's: a restatement takes the coefficients from here).  TTS_ERR_INVALID: NULL;
 * TTS_ERR_UNSUPPORTED: a sampling rate outside 8000 .. 192000. */
int tts_loudness_filter(int sampling_rate, double coeffs[10]);
/* Host only: the samples c of a segment at this sampling rate, ceil((sampling_rate / 10) / 8); 0 outside 8000 .. 192000. */
int tts_loudness_segment(int sampling_rate);

/* ---- true-peak meter and look-ahead peak limiter -------------------------------------------- */
/* The true peak of B mono utterances after ITU-R BS.1770-4 Annex 2: the peak of the 4x oversampled signal (no reference
 * counterpart).  wav DEVICE [B][N]; n_samples: HOST int32 [B] or NULL (all N) -- samples at or behind n_samples[b] are never read.
 * For an utterance x[0 .. n), with x = (double)wav[b][i] and zeros outside 0 .. n - 1:
 *   y[4 i] = x[i]
 *   y[4 i + p] = h[p][0] * x[i - 5] + h[p][1] * x[i - 4] + ... + h[p][11] * x[i + 6],  p = 1 .. 3: the point i + p / 4
 * the first product, then one sum per further product in ascending tap order, every product and sum an individually rounded IEEE
 * double operation.  h (tts_true_peak_filter) is a Kaiser (beta = 4) windowed sinc; its phase 0 is the unit impulse exactly.
 *   true_peak[b]   = the largest finite |y|, 0 where there is none: never below sample_peak[b]
 *   sample_peak[b] = the largest finite |x|, 0 where there is none
 * A non-finite sample makes the interpolated points within its taps' reach non-finite; they are skipped.  The maxima are taken
 * on bit patterns: order-free.  true_peak DEVICE double [B], sample_peak DEVICE double [B] or NULL (8-byte aligned).  dBTP =
 * 20 log10(true_peak) is the host's to take.  Exactness: the bits of tests/limiter_oracle.py.  Independence: an utterance's
 * results are the bits of its B = 1 call.  No model needs to be loaded.  Asynchronous on the handle's stream (a fill per output
 * and one launch per 64 utterances); profile stage "limiter".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL wav or true_peak, B or N < 1, an n_samples[b] outside 1 .. N, a misaligned
 * buffer. */
int tts_true_peak(tts_handle_t h, const float* wav /* [B][N] */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
                  double* true_peak /* [B] */, double* sample_peak /* [B] or NULL */);
/* Host only, no handle and no device: h[phase][tap], 4 x 12, as the library designed them (sin and the Bessel series are the
 * host's: a restatement takes the taps from here).  TTS_ERR_INVALID: NULL. */
int tts_true_peak_filter(double coeffs[48]);

/* What tts_limit reports per utterance; every field is order-free.  16 bytes. */
typedef struct tts_limit_stats {
    int32_t over;      /* finite samples whose envelope a[i] is above the ceiling */
    int32_t limited;   /* finite samples with an applied gain g[i] < 1 */
    double min_gain;   /* the smallest g[i] among them; 1.0 if none */
} tts_limit_stats_t;
/* A look-ahead peak limiter, in place: c = ceiling > 0, L = lookahead in 0 .. tts_limit_max_lookahead() samples, oversample 1
 * (sample peaks) or 4 (the interpolated peaks of tts_true_peak).  For an utterance x[0 .. n):
 *   envelope       a[i] = |x[i]| (oversample 1), or the largest finite |y[4 i + p]|, p = 0 .. 3 (oversample 4); 0 where x[i] is
 *                  not finite.  Non-finite interpolated points are skipped.
 *   required gain  r[i] = 1 where a[i] <= c, else c / a[i]
 *   minimum        m[i] = min r[j] over |j - i| <= L, j in 0 .. n - 1
 *   smoothed gain  s[i] = (m[cl(i - L)] + m[cl(i - L + 1)] + ... + m[cl(i + L)]) / (2 L + 1), summed in ascending order from its
 *                  first term, cl(j) = min(max(j, 0), n - 1): a function of L, i and the utterance alone
 *   applied gain   g[i] = min(s[i], r[i])
 *   output         wav[b][i] keeps its bits where g[i] == 1 or x[i] is not finite; else it becomes
 *                  copysign(min(|(float)(g[i] * x[i])|, cf), x[i]), cf the largest float <= c
 * with correctly rounded double quotients, products and sums.  Every window s[i] averages contains i, so s[i] <= r[i] in real
 * arithmetic; the min and the clamp make |out[i]| <= cf exact for every finite sample.  A row whose envelope stays at or below c
 * comes back as its own bits (its tiles are read once and nothing is written).  With oversample 4 the bound is on the envelope:
 * the gain modulation moves the interpolated peaks a little, so the output's true peak is measured (tts_true_peak), not promised.
 * stats DEVICE [B] or NULL (8-byte aligned).  Samples at or behind n_samples[b] are neither read nor written; an utterance's
 * result is the bits of its B = 1 call.  Asynchronous on the handle's stream, no host wait: a fill and three launches per 64
 * utterances; the workspace is a copy of the rows, from which the tiles that changed are copied back, so no tile reads what
 * another wrote.  Profile stage "limiter".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL wav, B or N < 1, a ceiling that is not finite and positive, a lookahead
 * outside 0 .. tts_limit_max_lookahead(), an oversample other than 1 or 4, an n_samples[b] outside 1 .. N, a misaligned buffer. */
int tts_limit(tts_handle_t h, float* wav /* [B][N], in place */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
              double ceiling, int lookahead, int oversample, tts_limit_stats_t* stats /* [B] or NULL */);
/* Host only: the largest lookahead, 1024 samples. */
int tts_limit_max_lookahead(void);

/* ---- the equaliser: a cascade of second-order sections -------------------------------------- */
/* Kinds of tts_equalizer_design. */
#define TTS_EQ_LOWPASS 0
#define TTS_EQ_HIGHPASS 1
#define TTS_EQ_PEAK 2
#define TTS_EQ_LOWSHELF 3
#define TTS_EQ_HIGHSHELF 4
/* A cascade of n_sections = 1 .. tts_equalizer_max_sections() second-order sections over every utterance (no reference
 * counterpart).  A section is the five doubles b0 b1 b2 a1 a2, normalised by a0; a sample runs through the cascade in direct form
 * II transposed, section after section:
 *   y = b0 x + z1;   z1 = (b1 x - a1 y) + z2;   z2 = b2 x - a2 y;   the next section's x = y
 * every product and sum an individually rounded IEEE double operation, the state zero in front of an utterance's first sample, and
 * the last section's y rounded to float32 once.  The recurrence is sequential, so an utterance is cut into segments of 256 samples
 * (the cut does not depend on a sampling rate; csrc/equalizer_plan.h): pass 1 runs every segment but the last from the zero state
 * and keeps the 2 n_sections state values it ends in, e_i; pass 2 chains them, S_0 = 0 and
 *   S_{i+1}[r] = (((M[r][0] S_i[0] + M[r][1] S_i[1]) + M[r][2] S_i[2]) + ...) + e_i[r]
 * in ascending column order with e_i[r] last, M the transition of 256 samples of zero input (column j: the state the recurrence
 * ends in from the unit state j), which the device computes with the same recurrence in a small launch of its own; pass 3 runs
 * every segment again from S_i and writes the output.  The result is the bits of tests/equalizer_oracle.py, and within 2^-30 of
 * its largest |y| of the recurrence run without a cut (DESIGN.md has the measured figures).  A NaN or an infinite sample makes
 * the rest of its utterance NaN, as the recurrence does.
 * out may equal wav (in place); any other overlap is refused.  Samples at or behind n_samples[b] are neither read nor written,
 * every other element of out is written exactly once, and an utterance's result is the bits of its B = 1 call.  Asynchronous on
 * the handle's stream, no host wait, nothing uploaded: one launch for M and three per 64 utterances; the workspace is the segments'
 * states.  Profile stage "equalize".
 * TTS_ERR_INVALID, before anything is enqueued, in this order: a NULL wav, out or sos; B or N < 1; an n_samples[b] outside 1 .. N;
 * n_sections outside 1 .. tts_equalizer_max_sections(); a coefficient that is not finite; a section outside the stability
 * triangle (|a2| < 1 and |a1| < 1 + a2 are needed); a buffer that is not 4-byte aligned; out overlapping wav without being equal
 * to it. */
int tts_equalize(tts_handle_t h, const float* wav /* [B][N] */, float* out /* [B][N]; may equal wav */, int B, int N,
                 const int32_t* n_samples /* HOST [B] or NULL */, const double* sos /* HOST [n_sections][5] */, int n_sections);
/* Host only: one section by the bilinear transform in its tan form, K = tan(pi f0 / sr).  TTS_EQ_LOWPASS and TTS_EQ_HIGHPASS take
 * a Q (gain_db is not looked at); TTS_EQ_PEAK, TTS_EQ_LOWSHELF and TTS_EQ_HIGHSHELF a Q and a gain in dB: a peak reads gain_db at
 * f0, a shelf gain_db / 2 at f0, gain_db at its end of the band and 0 dB at the other.  One low-pass or high-pass section at Q =
 * 0.7071067811865476 is a 2nd-order Butterworth filter, two at Q = 0.5411961001461969 and 1.3065629648763766 a 4th-order one.
 * TTS_ERR_UNSUPPORTED: a sampling rate outside 8000 .. 192000, f0 / sr outside 1e-4 .. 0.49, a Q outside 0.1 .. 30, a gain outside
 * -40 .. +24 dB.  TTS_ERR_INVALID: another kind, a NULL pointer. */
int tts_equalizer_design(int kind, int sampling_rate, double f0_hz, double q, double gain_db, double* sos5_out);
/* Host only: the sections of a named profile at a sampling rate -- "telephony" (4th-order Butterworth high-pass at 300 Hz, then
 * low-pass at 3400 Hz: 4 sections), "small-speaker" (4th-order high-pass at 150 Hz and a +3 dB peak at 3 kHz, Q 1), "rumble"
 * (2nd-order high-pass at 20 Hz, Q 0.7071), "bright" (high shelf at 6 kHz, +3 dB), "warm" (high shelf at 6 kHz, -3 dB, and a low
 * shelf at 200 Hz, +2 dB).  Every preset is UNTUNED: nobody has listened to one.  TTS_ERR_UNSUPPORTED: the sampling rate, or a
 * corner that does not fit under 0.49 sr (tts_last_error(NULL) names it).  TTS_ERR_INVALID: an unknown name, a NULL pointer. */
int tts_equalizer_profile(const char* name, int sampling_rate, double* sos_out /* [8][5] */, int* n_sections_out);
/* Host only: the largest cascade, 8 sections. */
int tts_equalizer_max_sections(void);

/* ---- the dynamics compressor: an envelope follower and a gain computer ----------------------- */
/* The parameters of tts_compress, by value.  threshold_db in -80 .. 0 (dB re full scale); slope = 1 / ratio in 0 .. 1 (0: ratio
 * infinity, 1: no compression); knee_db in 0 .. 40, the whole width W of the soft knee around the threshold; makeup_db in -24 .. +24;
 * attack_coeff = aA and release_coeff = aR in [0, 1), the one-pole coefficients tts_compressor_design makes of times in ms. */
typedef struct {
    double threshold_db, slope, knee_db, makeup_db, attack_coeff, release_coeff;
} tts_compressor_t;
/* What tts_compress can tell of a row: the samples it held, those whose gain reduction r was below 0, the largest reduction -r in
 * dB (0: none) and the largest |out| (NaN passed over). */
typedef struct {
    int32_t n;
    int32_t reduced;
    float max_reduction_db;
    float peak_out;
} tts_compress_stats_t;
/* A feed-forward peak compressor over every utterance (no reference counterpart).  Per row, x the sample as a double, the states e1
 * and e zero in front of its first sample:
 *   v  = |x|, or 0 where x is not finite                     the detector's input
 *   e1 = max(v, aR e1)                                        the release: a peak held and let go
 *   e  = aA e + bA e1,  bA = 1 - aA rounded once             the attack: two products and a sum, each individually rounded
 *   L  = 20 log10(e),  d = L - threshold_db,  W = knee_db
 *   r  = 0 where 2 d <= -W;  (slope - 1) d where 2 d >= W;  (slope - 1) (d + W / 2)^2 / (2 W) between them
 *   out = float32(x * 10^((r + makeup_db) / 20)), rounded once; x's own bits where r + makeup_db is exactly 0
 * r is computed directly and never as a difference of levels, so e = 0 gives r = 0.  A NaN sample is NaN at its own position and
 * silence to the detector; an infinite one stays infinite.  The recurrences are sequential, so an utterance is cut into the
 * equaliser's segments of 256 samples (csrc/compressor_plan.h): both maps compose in closed form over a segment, e1 -> max(c, AR e1)
 * and e -> AA e + q with AR and AA the coefficients multiplied out 256 times on the host.  Pass A keeps c of every segment but the
 * last, a chain makes the e1 every segment starts from, pass B keeps q (which depends on that e1), a second chain makes the e, and
 * pass C writes.  envelope is the bits of tests/compressor_oracle.py and within 2^-30 of its largest value of the recurrence run
 * without a cut; out is within 2^-24 |y| + 2^-40 |y| + 2^-150 of that oracle's double y.
 * out may equal wav (in place); any other overlap is refused.  Samples at or behind n_samples[b] are neither read nor written, every
 * other element of out is written exactly once, and an utterance's result is the bits of its B = 1 call.  envelope: DEVICE [B][N]
 * doubles, e of every sample, or NULL.  stats: DEVICE [B] records, or NULL.  Asynchronous on the handle's stream, no host wait,
 * nothing uploaded: five launches per 64 utterances, a sixth where records are asked for.  Profile stage "compress".
 * TTS_ERR_INVALID, before anything is enqueued, in this order: a NULL wav, out or params; B or N < 1; an n_samples[b] outside 1 .. N;
 * a parameter outside its range (threshold, slope, knee, make-up, attack, release, in that order); a wav or out that is not 4-byte
 * aligned; an envelope that is not 8-byte aligned; out overlapping wav without being equal to it. */
int tts_compress(tts_handle_t h, const float* wav /* [B][N] */, float* out /* [B][N]; may equal wav */, int B, int N,
                 const int32_t* n_samples /* HOST [B] or NULL */, const tts_compressor_t* params /* HOST, read before the call returns */,
                 double* envelope /* [B][N] or NULL */, tts_compress_stats_t* stats /* [B] or NULL */);
/* Host only: the coefficients of an attack and a release time, exp(-1 / (ms * 1e-3 * sampling_rate)); 0 ms gives 0 (no smoothing).
 * TTS_ERR_UNSUPPORTED: a sampling rate outside 8000 .. 192000, a time outside 0 .. 10000 ms.  TTS_ERR_INVALID: a NULL pointer. */
int tts_compressor_design(int sampling_rate, double attack_ms, double release_ms, double* attack_coeff_out, double* release_coeff_out);
/* Host only: the parameters of a named profile at a sampling rate, as threshold / ratio / knee / attack / release / make-up --
 * "speech" (-18 dB, 3:1, 6 dB, 5 ms, 100 ms, +3 dB), "telephony" (-20 dB, 4:1, 6 dB, 3 ms, 80 ms, +6 dB), "small-speaker" (-24 dB,
 * 6:1, 10 dB, 2 ms, 60 ms, +8 dB).  Every preset is UNTUNED: nobody has listened to one.  TTS_ERR_UNSUPPORTED: the sampling rate.
 * TTS_ERR_INVALID: an unknown name, a NULL pointer. */
int tts_compressor_profile(const char* name, int sampling_rate, tts_compressor_t* params_out);

/* ---- the audio watermark: a keyed spread-spectrum carrier, embedded and detected -------------- */
/* The parameters of both stages, by value.  key: any 64 bits.  payload: its low payload_bits bits travel.  payload_bits = P in
 * 1 .. 32.  chip = L, the samples of a chip, even, 2 .. 16.  chips_per_symbol = C in 1 .. 65536.  strength = G in 0 .. 0.25, the
 * carrier's amplitude as a fraction of the local envelope (the detector does not read it, and checks it all the same).  The
 * defaults of the layers above -- L = 8, C = 64, P = 16, G = 0.02 -- are UNTUNED: no trained checkpoint was at hand and nobody has
 * listened. */
typedef struct {
    uint64_t key;
    uint32_t payload;
    int32_t payload_bits;
    int32_t chip;
    int32_t chips_per_symbol;
    double strength;
} tts_watermark_t;
/* What tts_watermark_embed can tell of a row: the samples it held, those that were marked (finite, under a non-zero G e) and the
 * largest |out| among the samples it held (NaN passed over). */
typedef struct {
    int32_t n;
    int32_t marked;
    float peak_out;
    int32_t spare;
} tts_watermark_embed_stats_t;
/* What tts_watermark_detect says of a row: the lowest offset d with the largest T, the samples the row held, score = T[offset],
 * energy = E[offset], and the payload read there (bit j set where S[offset][j] < 0). */
typedef struct {
    int32_t offset;
    int32_t n;
    int64_t score;
    int64_t energy;
    uint32_t payload;
    uint32_t spare;
} tts_watermark_detect_t;
/* The carrier at position p >= 0, the same for every row (a detector need not know which row it holds):
 *   q = p / L, u = q / C, j = u mod P
 *   c(q) = +1 where bit 63 of splitmix64's finaliser of key + 0x9E3779B97F4A7C15 (q + 1) is 0, else -1
 *   m(t) = +1 for t < L / 2, else -1        no DC, a peak near fs / L: in the telephone band for L = 8 at 22 050 Hz
 *   s(p) = c(q) m(p mod L) (1 - 2 bit_j(payload))
 * The block envelope of a row, blocks of 64 samples from its first: E[k] the largest |x| of the finite samples of block k (0
 * where there is none or the block lies outside the row), e[i] = min(E[k - 1], E[k], E[k + 1]) for the block k that holds i --
 * so the first and the last block of a row carry no mark, nor does the block ahead of an onset.
 * Embed: out[i] = float32(double(wav[i]) + (G double(e[i])) s(i)), every double operation individually rounded and one rounding
 * to float32.  A sample that is not finite, and one with G e[i] == 0 (-0.0 and everything at or behind n_samples[b] among
 * them), comes back as its own bits.  The result is the bits of tests/watermark_oracle.py.
 * out may equal wav (in place: only marked samples are written); any other overlap is refused; apart, every element of out is
 * written exactly once.  An utterance's result is the bits of its B = 1 call.  n_samples: HOST [B] lengths in 0 .. N, or NULL
 * (all N).  stats: DEVICE [B] records, or NULL.  Asynchronous on the handle's stream, no host wait, nothing uploaded, no
 * atomics: two launches per 64 utterances, a third where records are asked for.  Profile stage "watermark".
 * TTS_ERR_INVALID, before anything is enqueued, in this order: a NULL wav, out or params; B or N < 1; an n_samples[b] outside
 * 0 .. N; a parameter outside its range (payload_bits, chip, chips_per_symbol, strength, in that order); a wav or out that is
 * not 4-byte aligned; out overlapping wav without being equal to it. */
int tts_watermark_embed(tts_handle_t h, const float* wav /* [B][N] */, float* out /* [B][N]; may equal wav */, int B, int N,
                        const int32_t* n_samples /* HOST [B] or NULL */, const tts_watermark_t* params /* HOST, read before the call returns */,
                        tts_watermark_embed_stats_t* stats /* [B] or NULL */);
/* The search for the carrier in received rows that may have lost their first samples: D candidate offsets d = 0 .. D - 1, d the
 * carrier position of the row's first sample.  With e_r the block envelope of the received row r:
 *   v[i]    = clamp(rint(64 double(r[i]) / double(e_r[i])), -127, 127), ties to even; 0 where r[i] is not finite or e_r[i] == 0
 *   a_q(d)  = the sum of v[i] m((i + d) mod L) over the samples with (i + d) / L == q
 *   S[d][j] = the sum of c(q) a_q(d) over the chips of bit j;  E[d] = the sum of a_q(d)^2;  T[d] = the sum over j of |S[d][j]|
 * all of them integers, exact in int64, whatever the order.  records: DEVICE [B].  scores: DEVICE [B][D] int64, all of T, or
 * NULL.  sums: DEVICE [B][P] int64, S[offset][:], or NULL.  The chip sums are made once per phase d mod L and cross-correlated
 * with the signs, about N D / L multiply-adds a row (csrc/watermark.hip); the argmax runs on the device.  Asynchronous on the
 * handle's stream, no host wait, nothing uploaded: one launch and five per 64 utterances.  Profile stage "watermark".
 * TTS_ERR_INVALID, before anything is enqueued, in this order: a NULL wav, records or params; B or N < 1; an n_samples[b] outside
 * 0 .. N; a parameter outside its range, as above; D outside 1 .. tts_watermark_max_offsets(); a wav that is not 4-byte
 * aligned; records, scores or sums that are not 8-byte aligned. */
int tts_watermark_detect(tts_handle_t h, const float* wav /* [B][N] */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
                         const tts_watermark_t* params /* HOST, read before the call returns */, int D,
                         tts_watermark_detect_t* records /* [B] */, int64_t* scores /* [B][D] or NULL */, int64_t* sums /* [B][P] or NULL */);
/* Host only: the largest D, 4096. */
int tts_watermark_max_offsets(void);

/* ---- attention diagnostics: alignment statistics ------------------------------------------- */
/* What the decoder's alignments say about whether the sentence was read (no reference counterpart: the reference plots its
 * alignments, tacotron/model.py:552-598, and judges them by eye).  alignments DEVICE [n_steps_max][B][Ts] as the decoder
 * writes them.  For utterance b let S = n_steps[b], N = n_sent[b] and row_s = alignments[s][b][0 .. Ts) for s < S; all
 * comparisons are on the float32 values:
 *   pos[s]   = np.argmax(row_s[:N]): the lowest index of the maximum; if the slice holds a NaN, the index of the first NaN
 *   peak[s]  = row_s[pos[s]], the bits of that element (NaN where the argmax is a NaN)
 *   off[s]   = 1 if np.argmax(row_s[:Ts]) >= N (the whole padded row, the same NaN rule), else 0: the strongest weight of
 *              the step lies on padding
 *   end_step = the smallest s with pos[s] == N - 1, or -1;  E = end_step if it is >= 0, else S - 1: the spoken part is 0 .. E
 *   d[s]     = pos[s] - pos[s-1] for 1 <= s <= E
 *   durations[b][j] = #{s < S : pos[s] == j} for j < N, 0 for N <= j < Ts
 * and the record of the utterance, 56 bytes: */
typedef struct tts_alignment_stats {
    int32_t n_sent, n_steps;   /* N and S, as used */
    int32_t reached;           /* max_s pos[s] over s < S */
    int32_t end_step;          /* as above */
    int32_t backward;          /* #{s : d[s] < 0} */
    int32_t max_back;          /* max(0, max_s -d[s]) */
    int32_t max_jump;          /* max(0, max_s d[s]) */
    int32_t longest_stall;     /* the longest run of equal consecutive pos[s] within 0 .. E (1 when E == 0) */
    int32_t after_end;         /* #{s > end_step : pos[s] != N - 1}; 0 when end_step == -1 */
    int32_t off_text;          /* sum_s off[s] over s < S */
    int32_t skipped;           /* #{j < reached : durations[j] == 0} */
    int32_t reserved;          /* 0 */
    double focus_sum;          /* ((peak[0] + peak[1]) + peak[2]) + ... in ascending s, every addition an individually rounded
                                  IEEE double addition; NaN propagates.  Mean focus = focus_sum / S is the caller's to take. */
} tts_alignment_stats_t;
/* Everything but focus_sum is an integer and focus_sum has a fixed order: the record is the same bits whatever B is, wherever
 * the utterance sits in the batch and however the library cuts the work (the bits of tests/alignment_oracle.py); a NaN in one
 * utterance touches no other.  Columns at or behind n_sent[b] are read for off alone; steps at or behind n_steps[b] are never
 * read.  n_sent: HOST int32 [B] or NULL (all Ts); n_steps: HOST int32 [B] or NULL (all n_steps_max) -- the lengths travel in
 * the launches, nothing is uploaded.  stats DEVICE [B]; durations DEVICE int32 [B][Ts] or NULL; pos DEVICE int32
 * [B][n_steps_max] or NULL, -1 behind n_steps[b]; peak DEVICE float [B][n_steps_max] or NULL, 0 behind n_steps[b].
 * No model needs to be loaded.  Asynchronous on the handle's stream (2 launches per 64 utterances); profile stage "alignment".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL alignments or stats, B, Ts or n_steps_max < 1, an n_sent[b] outside
 * 1 .. Ts, an n_steps[b] outside 1 .. n_steps_max, a misaligned buffer (stats: 8 bytes, the others: 4). */
int tts_alignment_stats(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts,
                        const int32_t* n_sent /* HOST [B] or NULL = Ts */, const int32_t* n_steps /* HOST [B] or NULL = n_steps_max */,
                        tts_alignment_stats_t* stats /* DEVICE [B] */, int32_t* durations /* DEVICE [B][Ts] or NULL */,
                        int32_t* pos /* DEVICE [B][n_steps_max] or NULL */, float* peak /* DEVICE [B][n_steps_max] or NULL */);
/* The sentence lengths of padded ids: n_sent[b] = 1 + the largest j with ids[b][j] != pad_id, 1 when the whole row is padding.
 * ids DEVICE int32 [B][Ts], n_sent DEVICE int32 [B].  Asynchronous on the handle's stream (1 launch); profile stage
 * "alignment".  TTS_ERR_INVALID: a NULL or misaligned pointer, B or Ts < 1. */
int tts_text_lengths(tts_handle_t h, const int32_t* ids /* DEVICE [B][Ts] */, int B, int Ts, int pad_id, int32_t* n_sent /* DEVICE [B] */);

/* ---- timing marks: a monotonic alignment search ---------------------------------------------- */
/* When every token is spoken: the best monotone path through an alignment history (no reference counterpart).  The argmax
 * track of tts_alignment_stats is no segmentation -- it jumps back, and a token's steps need not be contiguous --; this is one:
 * a non-decreasing position per step that advances by at most J = max_jump (1 .. 15) tokens a step.  alignments DEVICE
 * [n_steps_max][B][Ts] as the decoder writes them.  For utterance b let S = n_steps[b] and N = n_sent[b]:
 *   weight   w(s, j), j < N: the float32 element's own bit pattern read as an unsigned integer where the element is greater
 *            than 0 (+Inf included); 0 where it is a NaN, a zero of either sign or negative.  For positive floats that is a
 *            monotone piecewise-linear log2 scaled by 2^23: the path of the largest sum is the path of the largest product
 *            of weights up to 0.086 octave per factor, with no transcendental function and no rounding
 *   table    int64, unreachable cells -1:  D[0][j] = w(0, j) for j <= min(J, N - 1);
 *            D[s][j] = w(s, j) + max over 0 <= d <= min(J, j) of D[s-1][j-d] over the reachable predecessors (none: the cell
 *            is unreachable); among equal predecessors the smallest d wins and is d(s, j)
 *   path     last = the lowest j that maximises D[S-1][.];  q[S-1] = last, q[s-1] = q[s] - d(s, q[s])
 *   start    start[b][j] = #{s < S : q[s] < j} for 0 <= j <= N, and S for N < j <= Ts: token j is spoken during the steps
 *            [start[j], start[j+1])
 *   path     path[b][s] = q[s], -1 at or behind S
 * and the record of the utterance, 32 bytes: */
typedef struct tts_token_times_stats {
    int64_t score;             /* D[S-1][last] */
    int32_t n_sent, n_steps;   /* N and S, as used */
    int32_t last;              /* as above */
    int32_t jumps;             /* #{s >= 1 : q[s] - q[s-1] > 1}, plus 1 if q[0] > 1 */
    int32_t skipped;           /* #{j < last : start[j+1] == start[j]}: tokens the path gives no step */
    int32_t agree;             /* #{s < S : q[s] == pos[s]}, pos the argmax of tts_alignment_stats */
} tts_token_times_stats_t;
/* Every quantity is an integer and every sum exact: the result is the same bits whatever B is, wherever the utterance sits in
 * the batch and however the library cuts the work (the bits of tests/marks_oracle.py); a NaN in one utterance touches no
 * other.  Columns at or behind n_sent[b] and steps at or behind n_steps[b] are never read.  n_sent: HOST int32 [B] or NULL (all
 * Ts); n_steps: HOST int32 [B] or NULL (all n_steps_max) -- the lengths travel in the launches, nothing is uploaded.  start
 * DEVICE int32 [B][Ts + 1]; path DEVICE int32 [B][n_steps_max] or NULL; stats DEVICE [B].  No model needs to be loaded.
 * Asynchronous on the handle's stream (2 launches per 64 utterances: the positions, then one workgroup per utterance that
 * fills the table row by row and walks back); profile stage "alignment".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL alignments, start or stats, B, Ts or n_steps_max < 1, an n_sent[b]
 * outside 1 .. Ts, an n_steps[b] outside 1 .. n_steps_max, a max_jump outside 1 .. 15, a misaligned buffer (stats: 8 bytes, the
 * others: 4).  TTS_ERR_UNSUPPORTED: Ts above tts_token_times_max_tokens(). */
int tts_token_times(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts,
                    const int32_t* n_sent /* HOST [B] or NULL = Ts */, const int32_t* n_steps /* HOST [B] or NULL = n_steps_max */,
                    int max_jump, int32_t* start /* DEVICE [B][Ts + 1] */, int32_t* path /* DEVICE [B][n_steps_max] or NULL */,
                    tts_token_times_stats_t* stats /* DEVICE [B] */);
/* Host only: the most tokens Ts of a call, 1024. */
int tts_token_times_max_tokens(void);

/* ---- the join: an edit list over the rows of a waveform batch ------------------------------- */
/* Pieces of the rows of wav DEVICE [B][N], laid one behind the other into the rows of out DEVICE [G][N_out], with pauses or
 * cross-fades between them (no reference counterpart: the reference writes one file per line and stops at max_iterations
 * frames).  Piece p is samples [first, first + count) of row `row`; a row may be used any number of times, or never, in any
 * order.  group[p] (HOST int32 [P]) is the output row of piece p: non-decreasing over 0 .. G - 1, no group empty.
 *   layout   within a group piece p starts at output offset o[p]: 0 for the group's first piece, o[p+1] = o[p] + count[p] +
 *            gap[p]; the group is n_out[g] = o[last] + count[last] samples long, and the gap of a group's last piece is ignored.
 *   fades    piece p fades over f_p = min(fade, count[p] / 2) samples (integer division) at either edge: the gain of its sample i
 *            is s((2 i + 1) / (2 f_p)) for i < f_p, s((2 (count - 1 - i) + 1) / (2 f_p)) for i >= count - f_p and 1 elsewhere,
 *            with s(t) = (t * t) * (3.0 - 2.0 * t).  Numerator and denominator are exact integers converted to double, and
 *            every operation is an individually rounded IEEE double operation.
 *   overlap  a negative gap lays the head of piece p + 1 over the tail of piece p -- a cross-fade, s(t) + s(1 - t) being 1 up to
 *            rounding.  -gap[p] <= min(f_p, f_p+1) is required, so no output sample has more than two contributors and every
 *            overlap lies inside both fades.
 *   samples  with two contributors, out = (float)((double)x_a * w_a + (double)x_b * w_b), the earlier piece first, each product
 *            and the sum individually rounded, one rounding to float; with one contributor of gain w != 1, (float)((double)x * w);
 *            with one contributor of gain 1 the source's bits.  Gap samples and [n_out[g], N_out) are +0.0.  A NaN source sample
 *            is NaN in exactly the output samples it contributes to.
 * Every element of out[G][N_out] is written exactly once per call: no atomics, no memset, nothing read from out; the result
 * depends neither on what the handle ran before nor on how the list is cut into launches (the bits of tests/join_oracle.py).
 * The list travels by value, 128 pieces per launch: a call makes ceil(P / 128) launches, uploads nothing and waits for nothing.
 * Asynchronous on the handle's stream, no model needed; profile stage "join".
 * TTS_ERR_INVALID with a message, before anything is enqueued: a NULL pointer; B, N, P or G < 1; fade < 0 or above
 * tts_join_max_fade(); P above tts_join_max_pieces(); G above P; a row outside 0 .. B - 1, a first outside 0 .. N - 1, a count outside
 * 1 .. N - first; a group list that does not start at 0, decreases, skips a group or does not end at G - 1; a gap below
 * -min(f_p, f_p+1); N_out below the largest n_out[g] or G * N_out above 2^33; a misaligned buffer (4 bytes). */
typedef struct tts_join_piece {
    int32_t row, first, count, gap;
} tts_join_piece_t;   /* HOST */
/* Host only, no handle and no device: the checks of the list, and every group's length (tts_last_error(NULL) has the reason of
 * a refusal). */
int tts_join_plan(const tts_join_piece_t* pieces, int P, const int32_t* group /* HOST [P] */, int G, int B, int N, int fade,
                  int64_t* n_out /* HOST [G] */);
int tts_join(tts_handle_t h, const float* wav /* DEVICE [B][N] */, int B, int N, const tts_join_piece_t* pieces, int P,
             const int32_t* group /* HOST [P] */, int G, int fade, int N_out, float* out /* DEVICE [G][N_out] */);
/* Host only: the most pieces a call takes (4096), the longest fade in samples (2^20), and the output samples a workgroup
 * writes (512). */
int tts_join_max_pieces(void);
int tts_join_max_fade(void);
int tts_join_tile(void);

/* ---- prosody: a segment-wise warp of magnitude spectrograms ---------------------------------- */
/* An edit list over the frames of mag DEVICE [B][F][T], written to out DEVICE [B][F][T_out] -- the layout tts_denorm_power writes
 * and tts_griffin_lim_ragged reads (no reference counterpart: tts_stretch_magnitudes with a rate, a gain and pauses that vary
 * along the utterance).  Segment s is either speech -- source frames [first, first + frames) of row `row`, frames >= 1 and pause
 * == 0 -- or a pause -- frames == 0 and pause >= 1 output frames of silence; first, step and gain of a pause are ignored.  The
 * segments of a row are consecutive in the list, rows non-decreasing over 0 .. B - 1, no row without a segment; the speech segments
 * of a row may use any source range inside n_frames[row] (HOST int32 [B], or NULL: all T), in any order, any number of times.
 *   lengths  count[s] = ceil(frames * 65536 / step) (int64, exact) for speech, `pause` for a pause; within a row segment s starts
 *            at output frame o[s], the sum of the counts of the row's earlier segments, and the row holds n_out[row] = the sum of
 *            all of them.
 *   speech   output frame o + j, j < count: p = j * step (int64), i = first + (p >> 16), a = (p & 65535) * 2^-16 (exact),
 *            out[:, o + j] = (float)(g * ((1 - a) * x[:, i] + a * x[:, i + 1])), g = (double)gain: every product and sum an IEEE
 *            double operation rounded on its own (no FMA), one rounding to float32.  x[:, i + 1] reads as 0.0 where i + 1 >=
 *            n_frames[row] and is then never fetched; otherwise it is the row's next source frame, whichever segment that lies
 *            in.  The blend is always evaluated: 0 * NaN and 0 * Inf stay NaN, as in tts_stretch_magnitudes.
 *   zeros    the output frames of a pause and frames n_out[row] .. T_out - 1 are +0.0.
 * One whole-row segment {b, 0, n_frames[b], 0, q, 1.0f} per row is tts_stretch_magnitudes at rate q / 65536: the same lengths and
 * the same bits.  Every element of out is written exactly once per call: no atomics, no memset, nothing read from out; a row's
 * output is the same bits whatever B is and wherever the row sits in the batch, and however the list is cut into launches (the
 * bits of tests/warp_oracle.py).  The list travels by value, 64 segments per launch: a call makes ceil(S / 64) launches, uploads
 * nothing and waits for nothing.  Asynchronous on the handle's stream, no model needed; profile stage "warp".
 * TTS_ERR_INVALID with a message that names the segment or row, before anything is enqueued, in this order: a NULL pointer; B, F,
 * T or S < 1; S above tts_warp_max_segments(); B above S; an n_frames[b] outside 1 .. T; rows that do not start at 0, decrease, skip a row or
 * do not end at B - 1; then per segment a negative frames or pause, a segment that is both a pause and speech or neither, a speech
 * segment outside [0, n_frames[row]), a step outside 16384 .. 262144, a gain that is not finite or lies outside 0 .. 16; T_out
 * below the largest n_out[b] or above 2^30; a misaligned buffer (4 bytes). */
typedef struct tts_warp_segment {
    int32_t row, first, frames, pause;
    uint32_t step;   /* source frames per output frame, times 65536 */
    float gain;
} tts_warp_segment_t;   /* HOST, 24 bytes */
/* Host only, no handle and no device: the checks of the list, and every row's length (tts_last_error(NULL) has the reason of a
 * refusal). */
int tts_warp_plan(const tts_warp_segment_t* segments, int S, int B, int T, const int32_t* n_frames /* HOST [B] or NULL */,
                  int64_t* n_out /* HOST [B] */);
int tts_warp_magnitudes(tts_handle_t h, const float* mag /* DEVICE [B][F][T] */, int B, int F, int T,
                        const int32_t* n_frames /* HOST [B] or NULL */, const tts_warp_segment_t* segments, int S, int T_out,
                        float* out /* DEVICE [B][F][T_out] */);
/* Host only: the most segments a call takes (4096), and the output frames of a segment one workgroup writes (64, in 32 bins). */
int tts_warp_max_segments(void);
int tts_warp_tile(void);

/* ---- per-word pitch: a segment-wise resampler behind Griffin-Lim ----------------------------- */
/* An edit list over the samples of wav DEVICE [B][n], written to out DEVICE [B][N_out] (no reference counterpart: tts_resample with
 * a ratio that varies along the utterance; behind tts_warp_magnitudes and Griffin-Lim it gives a word its own pitch and leaves its
 * duration alone).  Segment s takes source samples [first, first + samples) of row `row`, samples >= 1, at `ratio` output samples per
 * input sample.  The segments of a row are consecutive in the list, rows non-decreasing over 0 .. B - 1, no row without a segment;
 * the segments of a row may use any source range inside n_samples[row] (HOST int32 [B], or NULL: all n), in any order, any number
 * of times.
 *   lengths    count[s] = samples where ratio == 1.0 exactly (a COPY), else (long long)(samples * ratio), the product in double,
 *              truncated (resampy's; it may be 0); within a row segment s starts at output sample o[s], the sum of the counts of the
 *              row's earlier segments, and the row holds n_out[row] = the sum of all of them.
 *   copy       out[row][o + j] = the bits of wav[row][first + j], j < count: NaN payloads and -0.0 survive.
 *   resampled  output sample o + j, j < count, is tts_resample's arithmetic with the position measured from `first`: with scale,
 *              step, inc, win and delta of `ratio` as above (see "resampling"),
 *                tr = j inc, m = first + (long long)tr, frac = scale (tr - (long long)tr);   f = 512 frac, off = (int)f, eta = f - off
 *                y  = sum_i fma(eta, delta[off + i step], win[off + i step]) x[m - i]          i < (32769 - off) / step
 *                   + the same with frac = scale - frac on x[m + 1 + k]                        k < (32769 - off) / step
 *              the position in double, every operation rounded on its own; the left wing with i ascending, then the right wing
 *              with k ascending, each tap an FMA into ONE accumulator that starts at 0.0, in double, rounded once to float32.  x is
 *              the ROW: the taps reach over the segment's borders into the row's own samples, whichever segment those lie in, and
 *              are cut only at the row's ends -- a sample outside [0, n_samples[row]) is 0.0 and is never fetched.  A NaN or Inf
 *              sample reaches every output whose window covers it and no other.
 *   zeros      samples n_out[row] .. N_out - 1 are +0.0.
 * One whole-row segment {b, 0, n_samples[b], 0, ratio} per row, ratio != 1, is tts_resample at that ratio with N_out: the same
 * lengths and the same bits.  Every element of out is written exactly once per call: no atomics, no memset, nothing read from out;
 * a row's output is the same bits whatever B is and wherever the row sits in the batch, and however the list is cut into launches
 * (within tests/resample_segments_oracle.py's float64 by resample_oracle's bound).  The list travels by value, 64 segments per
 * launch: a call makes at most ceil(S / 64) launches (a launch whose segments own no sample is not made) and waits for nothing.
 * Ratios of 1 and above share one table; each distinct ratio below 1 has a table of its own (0.5 MiB, kept on the handle), at
 * most tts_resample_segments_max_ratios() of them per call.  The FIRST use of a ratio below 1 builds its table on the host and
 * uploads it with a synchronous copy, which blocks the calling thread, as in tts_resample; and a call whose new tables do not fit
 * beside the 32 the handle keeps synchronises the handle's streams once and drops the kept ones before it fetches its own.
 * Otherwise asynchronous on the handle's stream, no model needed; profile stage "resample".  n_out: HOST int32 [B], the rows'
 * lengths, or NULL.
 * TTS_ERR_INVALID with a message that names the segment or row, before anything is enqueued, in this order: a NULL pointer (wav,
 * segments, out); B, n, S or N_out < 1; S above tts_resample_segments_max(); B above S; an n_samples[b] outside 1 .. n; rows that
 * do not start at 0, decrease, skip a row or do not end at B - 1; then per segment samples < 1, first < 0 or first + samples
 * beyond n_samples[row], a ratio that is not finite or lies outside [0.25, 4], reserved != 0; more than
 * tts_resample_segments_max_ratios() distinct ratios below 1; N_out below the largest n_out[b] or above 2^30; a misaligned buffer
 * (4 bytes). */
typedef struct tts_resample_segment {
    int32_t row, first, samples, reserved;   /* reserved must be 0 */
    double ratio;                            /* output samples per input sample */
} tts_resample_segment_t;   /* HOST, 24 bytes */
/* Host only, no handle and no device: the checks of the list, and every row's length (tts_last_error(NULL) has the reason of a
 * refusal). */
int tts_resample_segments_plan(const tts_resample_segment_t* segments, int S, int B, int n, const int32_t* n_samples /* HOST [B] or NULL */,
                               int64_t* n_out /* HOST [B] */);
int tts_resample_segments(tts_handle_t h, const float* wav /* DEVICE [B][n] */, int B, int n, const int32_t* n_samples /* HOST [B] or NULL */,
                          const tts_resample_segment_t* segments, int S, int N_out, float* out /* DEVICE [B][N_out] */,
                          int32_t* n_out /* HOST [B] or NULL */);
/* Host only: the most segments a call takes (4096), the most distinct ratios below 1 among them (16), and the output samples of a
 * segment one workgroup writes (256). */
int tts_resample_segments_max(void);
int tts_resample_segments_max_ratios(void);
int tts_resample_segments_tile(void);

/* ---- formant-preserving pitch: a cepstral-envelope shift of magnitude spectrograms ------------ */
/* An edit list over the frames of mag DEVICE [B][F][T], written to out DEVICE [B][F][T] -- the layout tts_denorm_power writes and
 * tts_warp_magnitudes reads (no reference counterpart: the reference's pitch_shift resamples, which moves the formants with the
 * pitch).  F = N + 1 with N a power of two, 128 .. 2048.  Segment s covers the frames [first, first + frames) of row `row`, frames
 * >= 1.  The segments of a row are consecutive in the list, rows non-decreasing over 0 .. B - 1, no row without a segment; within a
 * row the ranges ascend, do not overlap and lie inside n_frames[row] (HOST int32 [B], or NULL: all T).  Durations do not change.
 *   copies    a frame below n_frames[row] that no segment covers, and every frame of a segment whose two steps are both 65536,
 *             is the bits of mag: NaN payloads and -0.0 survive.
 *   zeros     frames t >= n_frames[row] are never read and are written as +0.0.
 *   computed  every other frame, with x[k] = (double)mag[row][k][t], k = 0 .. N, and Q = order:
 *               L[k]  = log(max(x[k], 1e-10))                           (a NaN x[k] gives a NaN L[k])
 *               c[q]  = (1 / N) sum_k w[k] L[k] ct[(q k) mod 2N]        q < Q; w[0] = w[N] = 1/2, else 1; ct[j] = cos(pi j / N), built
 *                                                                       on the host in double
 *               E[k]  = sum_{q < Q} h[q] c[q] ct[(q k) mod 2N]          h[0] = 1, h[q] = 1 + cos(pi q / Q): a raised-cosine lifter,
 *                                                                       built on the host in double
 *               X[k]  = x[k] exp(-E[k])                                 the fine structure (x itself, not the floored value)
 *               p  = k * pitch_step (int64); if p > N << 16: p = (2N << 16) - p   (the band above Nyquist is filled by folding)
 *               i  = p >> 16, a = (p & 65535) * 2^-16;    Xs[k] = (1 - a) X[i] + a X[min(i + 1, N)]
 *               p' = min(k * formant_step, N << 16), i', a' likewise;   Ew[k] = (1 - a') E[i'] + a' E[min(i' + 1, N)]
 *               out[row][k][t] = (float)(exp(Ew[k]) Xs[k])              in double, rounded once
 *             The order of the sums is not prescribed (it depends on N and order alone); the result is within
 *             2^-24 |y| + eta (|t1| + |t2|) of the same formulas in float64 (tests/shift_oracle.py), t1 and t2 the two terms of the
 *             blend of Xs times exp(Ew), eta = 2^-53 * 8 Q (F + 2) (1 + max |L|).  An all-zero frame gives +0.0
 *             exactly; a frame that holds a NaN or an Inf comes out all NaN and touches no other frame; the sign of a negative input
 *             follows x.
 * Every element of out is written exactly once per call: no atomics, no memset, nothing read from out; a row's output is the same
 * bits whatever B is and wherever the row sits in the batch, and however the list is cut into launches.  The list travels by value,
 * 64 segments per launch: a call makes ceil(S / 64) launches.  ct (2N doubles) is kept on the handle per N and the lifter per
 * order: the FIRST use of an N or an order builds its table on the host and uploads it with a synchronous copy; otherwise the call
 * is asynchronous on the handle's stream and waits for nothing.  No model needed; profile stage "shift".
 * TTS_ERR_INVALID with a message that names the segment or row, before anything is enqueued, in this order: a NULL pointer (mag,
 * segments, out); out == mag; B, T or S < 1; an F that is not 2^m + 1 with 2^m in 128 .. 2048; order outside 2 ..
 * min(tts_shift_max_order(), N / 2); S above tts_shift_max_segments(); B above S; an n_frames[b] outside 1 .. T; rows that do not
 * start at 0, decrease, skip a row or do not end at B - 1; then per segment frames < 1, a range outside [0, n_frames[row]), a range
 * that starts in front of its predecessor's end, reserved != 0, a pitch_step and then a formant_step outside 32768 .. 131072 (one
 * octave either way); a misaligned buffer (4 bytes). */
typedef struct tts_shift_segment {
    int32_t row, first, frames, reserved;   /* reserved must be 0 */
    uint32_t pitch_step;    /* source bins per output bin of the fine structure, times 65536: round(65536 / rho) */
    uint32_t formant_step;  /* source bins per output bin of the envelope, times 65536: round(65536 / phi) */
} tts_shift_segment_t;   /* HOST, 24 bytes */
/* Host only, no handle and no device: the checks of the shape, the order and the list (tts_last_error(NULL) has the reason of a
 * refusal). */
int tts_shift_plan(const tts_shift_segment_t* segments, int S, int B, int F, int T, const int32_t* n_frames /* HOST [B] or NULL */, int order);
int tts_shift_magnitudes(tts_handle_t h, const float* mag /* DEVICE [B][F][T] */, int B, int F, int T,
                         const int32_t* n_frames /* HOST [B] or NULL */, const tts_shift_segment_t* segments, int S, int order,
                         float* out /* DEVICE [B][F][T], not mag */);
/* Host only: the most segments a call takes (4096), the frames of a computed segment one workgroup takes (8), and the largest
 * order (256). */
int tts_shift_max_segments(void);
int tts_shift_tile(void);
int tts_shift_max_order(void);

/* ---- delivery formats: 16-bit PCM, 8-bit PCM and G.711 --------------------------------------- */
#define TTS_FMT_F32 0        /* float32 as the library makes it: no encoding */
#define TTS_FMT_PCM_S16 1    /* signed 16-bit PCM, 2 bytes per code */
#define TTS_FMT_PCM_U8 2     /* unsigned 8-bit PCM (WAV's), offset 128 */
#define TTS_FMT_MULAW 3      /* ITU-T G.711 mu-law, 1 byte per code */
#define TTS_FMT_ALAW 4       /* ITU-T G.711 A-law, 1 byte per code */
#define TTS_DITHER_NONE 0
#define TTS_DITHER_TPDF 1    /* triangular, (-1, 1) LSB, added before the rounding */
/* What tts_encode reports per row; every field is order-free.  16 bytes. */
typedef struct tts_encode_stats {
    int32_t clipped;   /* samples whose rounded value lay outside the format's range (+-Inf included) and was saturated */
    int32_t nans;      /* NaN samples: encoded as zero */
    int32_t peak;      /* the largest |q| after saturation */
    int32_t n;         /* the samples the row holds: n_samples[b], or N */
} tts_encode_stats_t;
/* Float32 rows to delivery codes, one streaming pass (no reference counterpart).  wav DEVICE [B][N] (4-byte aligned); out
 * DEVICE [B][N] codes of tts_encode_width(format) bytes, rows N codes apart with no padding (aligned as a code is: 2 bytes for
 * TTS_FMT_PCM_S16); n_samples: HOST int32 [B] or NULL (all N), 0 .. N each.  Sample i < n_samples[b] of row b:
 *   scale   v = (double)x * Q, Q = 128 (PCM_U8) or 32768 (the others): exact
 *   dither  d = 0 (TTS_DITHER_NONE), or with TTS_DITHER_TPDF, in arithmetic modulo 2^64,
 *             z = seed + 0x9E3779B97F4A7C15 * (((uint64)b << 32 | i) + 1)
 *             z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *             d = ((double)(z >> 32) - (double)(z & 0xFFFFFFFF)) * 2^-32
 *           exact, triangular on (-1, 1) LSB, a function of (seed, b, i) alone: never of the tiling or the grid
 *   round   q = rint(v + d), ties to even.  A NaN gives q = 0 and counts in `nans`; q outside [-Q, Q - 1] (+-Inf included) is
 *           saturated and counts in `clipped`
 *   code    PCM_S16: q.  PCM_U8: q + 128.  MULAW / ALAW: ITU-T G.711 from the 16-bit q by the CCITT / Sun g711.c arithmetic, which
 *           Python's audioop.lin2ulaw(., 2) / lin2alaw(., 2) run: mu-law from q >> 2 (clip 8159, bias 33), A-law from q >> 3
 *           (negative magnitudes -v - 1).  Digital silence is 0xFF (mu-law) and 0xD5 (A-law).
 * Samples i >= n_samples[b] are written as the format's code for zero, undithered, and count nowhere: every code of out is
 * written by every call.  stats DEVICE [B] or NULL (4-byte aligned): peak the largest |q| after saturation, n = n_samples[b].
 * Exactness: the bits of tests/encode_oracle.py.  No model needs to be loaded.  Asynchronous on the handle's stream, no host wait:
 * two launches per 64 rows (the records, the pass); profile stage "encode".
 * TTS_ERR_INVALID, before anything is enqueued: a NULL wav or out, B or N < 1, an unknown format or TTS_FMT_F32 (no encoding), an
 * unknown dither, an n_samples[b] outside 0 .. N, a misaligned buffer. */
int tts_encode(tts_handle_t h, const float* wav /* DEVICE [B][N] */, int B, int N, const int32_t* n_samples /* HOST [B] or NULL */,
               int format, int dither, uint64_t seed, void* out /* DEVICE [B][N] codes */, tts_encode_stats_t* stats /* DEVICE [B] or NULL */);
/* Host only: the bytes of a code -- 2, 1, 1, 1 for the four encodings, 4 for TTS_FMT_F32; negative for an unknown format. */
int tts_encode_width(int format);
/* Host only: the samples of a row one workgroup takes. */
int tts_encode_tile(void);

/* ---- end to end -------------------------------------------------------------------------- */
/* ids -> waveform: encoder, decoder (n_steps), post-net, de-normalise, ** power, Griffin-Lim,
 * optional peak normalisation; replaces tacotron/inference.py:162-200 minus file IO.
 * Optional outputs (NULL to skip): mel [B*n_steps*r*n_mels], alignments [n_steps*B*Ts],
 * linear [B*T*F].  wav [B * hop*(T-1)], T = n_steps*reduction. */
typedef struct tts_synth_params {
    int32_t n_steps;        /* 200 */
    float ref_db, max_db;   /* 6.02, 99.89 (mel constants, as the reference uses them) */
    float power;            /* 1.3 */
    int32_t n_iter;         /* 50 */
    int32_t win_length, hop_length;  /* 1102, 275 */
    uint64_t seed;          /* random initial phase when init_phase == NULL */
    int32_t peak_normalize; /* save_wav(norm=True) */
    int32_t host_outputs;   /* tts_synthesize_host only: TTS_HOST_* flags of what travels to host memory besides the
                               waveforms (0 = nothing); ignored by tts_synthesize, whose optional outputs are pointers */
} tts_synth_params_t;
#define TTS_HOST_LINEAR 1       /* linear spectrograms [B*T*F]: what the reference's inference() hands back (tacotron/inference.py:75-101) */
#define TTS_HOST_ALIGNMENTS 2   /* alignments [n_steps*B*Ts] (tacotron/model.py:552-598 dumps them) */
int tts_synthesize(tts_handle_t h, const int32_t* ids, int B, int Ts, const tts_synth_params_t* p,
                   const float* init_phase /* [B*F*T] or NULL */, float* wav, float* mel,
                   float* alignments, float* linear);

/* The same call for a caller that lives in HOST memory -- what the reference's inference() / serve() are
 * (tacotron/inference.py:75-101,185-200, serve.py:89-126: host id arrays in, host waveforms out) -- without giving up the
 * call pipeline: the ids are copied to a pinned staging buffer of the handle and uploaded on the stream that runs
 * the call's encoder, in front of it (the initial phases are drawn on the device from p->seed, as the reference
 * draws them with np.random), and the waveforms are downloaded into pinned memory of the handle on a copy
 * stream as soon as they are complete.  The call returns at once with a ticket; tts_wait_host blocks until that
 * call's waveforms have arrived and hands out the pinned buffer, [B * hop*(T-1)] floats, valid until the THIRD
 * tts_synthesize_host call after the one that produced it (three buffer sets rotate: the device holds three calls at
 * once -- the encoder of call k + 2, the decoder of k + 1, the post-net / Griffin-Lim of k).  Keep at most three calls in
 * flight: submit k + 2, then wait for k.  Bit-identical to tts_synthesize + tts_memcpy_d2h. */
int tts_synthesize_host(tts_handle_t h, const int32_t* ids_host, int B, int Ts, const tts_synth_params_t* p,
                        int* ticket);
int tts_wait_host(tts_handle_t h, int ticket, const float** wav_host, size_t* n_floats);
/* The optional outputs of the same call (p->host_outputs), in pinned memory of the handle with the lifetime of the
 * waveform buffer: linear spectrograms [B][T][F] as the network emits them (normalised dB, before the de-normalisation),
 * alignments [n_steps][B][Ts].  Pointers are NULL / counts 0 for outputs the call did not ask for.  Waits like
 * tts_wait_host (and reports what it reports); the waveforms are fetched with tts_wait_host itself. */
int tts_wait_host_outputs(tts_handle_t h, int ticket, const float** linear_host, size_t* n_linear, const float** align_host,
                          size_t* n_align);

/* Stop where the speech ends (the reference's TODO, tacotron/inference.py:76-78).  A setting of the HANDLE, off by default and
 * read when a call is made (as "gl_momentum" is): with enabled != 0, tts_synthesize and tts_synthesize_host run
 * tts_speech_frames on the call's de-normalised magnitudes behind the post-net -- threshold_db converted with the call's
 * power (tts_speech_threshold, TTS_SPEECH_MAGNITUDE_POWER; the call's ref_db / max_db de-normalised the data), keep_frames
 * as given, min_frames = the smallest n with hop (n - 1) > n_fft / 2 -- WAIT on the host for the B lengths (the call then
 * returns once its post-net has run; its Griffin-Lim, and the next call's decoder beside it, are asynchronous as ever) and
 * reconstruct every utterance from its first n_frames[b] frames alone, as tts_griffin_lim_ragged does: wav keeps its shape
 * [B][hop (T - 1)], samples [0, hop (n_frames[b] - 1)) are utterance b and the rest of the row is 0; with peak_normalize each
 * utterance is scaled by its own peak (the bits of tts_peak_normalize on the padded rows).  mel / alignments / linear stay
 * full length.  Lengths that all equal T give the bits of the call with the setting off.  A call whose T is below min_frames
 * is TTS_ERR_INVALID.  The decoder loop itself always runs n_steps steps.
 * TTS_ERR_INVALID (the setting stays as it was): a NaN threshold_db, keep_frames < 0. */
int tts_set_end_of_speech(tts_handle_t h, int enabled, float threshold_db, int keep_frames);
/* The lengths of the last tts_synthesize / tts_synthesize_host call made on the handle: n_frames_host, HOST int32 [B] (B: that
 * call's; TTS_ERR_INVALID otherwise, or when no call has been made).  All T for a call made with the setting off.  Host only:
 * the call itself has read them. */
int tts_synth_frames(tts_handle_t h, int32_t* n_frames_host, int B);
/* The lengths of a tts_synthesize_host call: waits as tts_wait_host does (same ticket rules, same reports), then hands out
 * the handle's host copy, valid as long as the ticket's waveform buffer. */
int tts_wait_host_frames(tts_handle_t h, int ticket, const int32_t** n_frames, int* B);

/* The speaking rate of synthesis (the reference's time_stretch, audio/effects.py:46-88, moved ahead of the one Griffin-Lim a call
 * runs anyway).  A setting of the HANDLE, read when a call is made (as "gl_momentum" and tts_set_end_of_speech are); the default
 * 1.0 means off, and off is the call as it always was, launch for launch.  With another rate tts_synthesize and
 * tts_synthesize_host time-stretch the call's de-normalised magnitude ** power rows behind the post-net (tts_stretch_rows: exactly
 * what Griffin-Lim consumes -- the blend acts on |S| ** power, the array the call has) and reconstruct from
 * T' = tts_stretched_frames(T, rate) frames: wav is [B][hop (T' - 1)], an init_phase argument [B][F][T'], the pinned buffers of
 * the host form are sized for T'; mel, alignments and linear keep their full length T.  The host form stays bit-identical to
 * tts_synthesize + tts_memcpy_d2h; "gl_momentum" composes unchanged.  With end-of-speech stopping the lengths n[b] are detected on
 * the unstretched magnitudes as ever and become n'[b] = min(T', max(min_frames, tts_stretched_frames(n[b], rate))) -- frames this
 * adds are the vocoder's zeros; the ragged Griffin-Lim and the per-utterance peak normalisation run on them as they do today,
 * and tts_synth_frames / tts_wait_host_frames report n'[b], the frames the waveform holds (all T' without stopping).  A call
 * with T' < min_frames (hop (n - 1) > n_fft / 2) is TTS_ERR_INVALID.  The first call after the rate changed is not pipelined
 * (its buffers grow).  The decoder loop always runs n_steps steps.
 * TTS_ERR_INVALID (the setting stays as it was): a rate that is not finite or outside [0.25, 4]. */
int tts_set_speaking_rate(tts_handle_t h, double rate);

/* The pitch of synthesis, in octaves (the reference's pitch_shift, audio/effects.py:9-43: a time-stretch by 2 ** -octaves, then
 * the resampler back to the length it had).  A setting of the HANDLE, read when a call is made; the default 0 means off, and off
 * is the call as it always was, launch for launch.  Otherwise, with rho = exp2(-octaves) and s the speaking rate,
 * tts_synthesize and tts_synthesize_host stretch the call's magnitudes by s rho (tts_stretch_rows) to
 * T' = tts_stretched_frames(T, s rho) frames, Griffin-Lim reconstructs hop (T' - 1) samples without peak normalisation, and
 * tts_resample takes them by rho into rows of hop (T_s - 1) samples, T_s = tts_stretched_frames(T, s); with peak_normalize
 * tts_peak_normalize then runs on those rows.  Pitch changes no shape and no reported length: wav, the pinned buffers and
 * tts_synth_frames / tts_wait_host_frames are those of the same call without pitch; only init_phase is [B][F][T'].  With
 * end-of-speech stopping the detection is as ever, the frames reported for utterance b stay n_s[b], the un-shifted call's,
 * Griffin-Lim runs on n'[b] = min(T', max(min_frames, tts_stretched_frames(n[b], s rho))) frames, and row b holds
 * min((long long)(hop (n'[b] - 1) rho), hop (n_s[b] - 1)) samples and zeros behind them.  A call whose s rho falls outside
 * [0.25, 4] or whose T' < min_frames is TTS_ERR_INVALID, and so is one whose T_s < min_frames (the call without pitch, whose
 * rows it fills, is refused too).  The first call after the setting changed is not pipelined; the first call at a new
 * 2 ** -octaves also builds that ratio's resampling table on the host (32 769 window samples, a Bessel series each, once per
 * handle, then 0.5 MiB per ratio) and uploads it with a synchronous copy: it blocks the calling thread for that long, also in
 * the middle of a stream of tts_synthesize_host calls.  A caller that switches pitch per request can pay that ahead of time
 * with a tts_resample call at each ratio it will use.
 * "gl_momentum" composes unchanged; the host form stays bit-identical to tts_synthesize + tts_memcpy_d2h.
 * TTS_ERR_INVALID (the setting stays as it was): a shift that is not finite or |octaves| > 1. */
int tts_set_pitch(tts_handle_t h, double octaves);

/* The loudness of synthesis: a target in LUFS after ITU-R BS.1770-4 (tts_loudness_normalize).  A setting of the HANDLE, off by
 * default and read when a call is made; off is the call as it always was, launch for launch.  With enabled != 0,
 * tts_synthesize and tts_synthesize_host do not peak-normalise, whatever p->peak_normalize says; they run
 * tts_loudness_normalize(target_lufs, max_peak) at sampling_rate on the call's final rows instead -- behind Griffin-Lim, or with
 * a pitch behind tts_resample -- on the call's stream, with no host wait.  Each utterance is measured over the samples its row
 * holds: hop (n[b] - 1) of the reported lengths with end-of-speech stopping (tts_synth_frames), all hop (T_s - 1) otherwise.  The
 * result is the bits of the same call made with peak_normalize = 0 followed by tts_loudness_normalize on those rows; the host
 * form stays bit-identical to tts_synthesize + tts_memcpy_d2h.  The first call after the setting was switched on is not
 * pipelined (its buffers are new).  sampling_rate is the caller's word for the model's rate: the library's configuration does
 * not carry one.
 * With enabled == 0 the other arguments are not looked at.  The setting stays as it was on TTS_ERR_INVALID (a target that is
 * not finite, a max_peak that is not finite and positive) and on TTS_ERR_UNSUPPORTED (a sampling rate outside 8000 .. 192000). */
int tts_set_loudness(tts_handle_t h, int enabled, double target_lufs, double max_peak, int sampling_rate);

/* The peak limiter of synthesis (tts_limit).  A setting of the HANDLE, off by default and read when a call is made; off is the
 * call as it always was, launch for launch.  With enabled != 0, tts_synthesize and tts_synthesize_host run
 * tts_limit(ceiling, lookahead, oversample) last on the call's final rows -- behind the loudness normaliser, or behind the peak
 * normalisation where there is no loudness target -- on the call's stream, with no host wait, over the samples each row holds
 * (the lengths the loudness setting uses).  The result is the bits of the same call made with the setting off followed by
 * tts_limit on those rows; the host form stays bit-identical to tts_synthesize + tts_memcpy_d2h.  The first call after the
 * setting was switched on is not pipelined (its buffers are new).
 * With enabled == 0 the other arguments are not looked at.  The setting stays as it was on TTS_ERR_INVALID (a ceiling that is
 * not finite and positive, a lookahead outside 0 .. tts_limit_max_lookahead(), an oversample other than 1 or 4). */
int tts_set_limiter(tts_handle_t h, int enabled, double ceiling, int lookahead, int oversample);

/* The equaliser of synthesis (tts_equalize).  A setting of the HANDLE, off by default and read when a call is made; off is the
 * call as it always was, launch for launch.  With enabled != 0, tts_synthesize and tts_synthesize_host run
 * tts_equalize(sos, n_sections) in place on the call's rows -- behind Griffin-Lim, the pitch resampler and the peak normalisation,
 * ahead of the loudness normaliser and the limiter -- on the call's stream, with no host wait, over the samples each row holds
 * (the lengths the loudness setting uses).  The sections are copied.  The result is the bits of the same call made with the
 * setting off followed by tts_equalize on those rows.  Lengths, shapes and timing marks do not change: the group delay of a few
 * samples is ignored.  A boost behind the peak normalisation can pass 1.0: give it a limiter or a loudness target.  The first
 * call after the setting was switched on is not pipelined (its buffers are new).
 * With enabled == 0 the other arguments are not looked at.  The setting stays as it was on TTS_ERR_INVALID (a NULL sos, n_sections
 * outside 1 .. tts_equalizer_max_sections(), a coefficient that is not finite, a section that is not stable). */
int tts_set_equalizer(tts_handle_t h, int enabled, const double* sos /* HOST [n_sections][5] */, int n_sections);

/* The compressor of synthesis (tts_compress).  A setting of the HANDLE, off by default and read when a call is made; off is the
 * call as it always was, launch for launch.  With enabled != 0, tts_synthesize and tts_synthesize_host run tts_compress(params) in
 * place on the call's rows -- behind the equaliser, ahead of the loudness normaliser and the limiter -- on the call's stream, with
 * no host wait, over the samples each row holds (the lengths the loudness setting uses).  The parameters are copied.  The result is
 * the bits of the same call made with the setting off followed by tts_compress on those rows.  Lengths, shapes and timing marks do
 * not change.  A make-up gain behind the peak normalisation can pass 1.0: give it a limiter or a loudness target.  The first call
 * after the setting was switched on is not pipelined (its buffers are new).
 * With enabled == 0 params is not looked at.  The setting stays as it was on TTS_ERR_INVALID (a NULL params, a parameter outside
 * its range). */
int tts_set_compressor(tts_handle_t h, int enabled, const tts_compressor_t* params);

/* The watermark of synthesis (tts_watermark_embed).  A setting of the HANDLE, off by default and read when a call is made; off is
 * the call as it always was, launch for launch.  With enabled != 0, tts_synthesize and tts_synthesize_host run
 * tts_watermark_embed(params) in place on the call's rows -- behind the compressor, ahead of the loudness normaliser and the
 * limiter, so the two gains scale the mark with the speech and the limiter's ceiling stays exact -- on the call's stream, with no
 * host wait, over the samples each row holds (the lengths the loudness setting uses).  The parameters are copied.  The result is
 * the bits of the same call made with the setting off followed by tts_watermark_embed on those rows.  Lengths, shapes and timing
 * marks do not change.  The first call after the setting was switched on is not pipelined (its buffers are new).
 * With enabled == 0 params is not looked at.  The setting stays as it was on TTS_ERR_INVALID (a NULL params, a parameter outside
 * its range). */
int tts_set_watermark(tts_handle_t h, int enabled, const tts_watermark_t* params);

/* Attention diagnostics of synthesis: the alignment statistics of every call (tts_alignment_stats).  A setting of the HANDLE,
 * off by default and read when a call is made; off is the call as it always was, launch for launch.  With enabled != 0,
 * tts_synthesize and tts_synthesize_host run tts_text_lengths(pad_id) on the call's device ids behind its encoder and
 * tts_alignment_stats (n_steps[b] = p->n_steps for every b, the sentence lengths read from device memory) right behind the
 * call's decoder, on the stream the decoder ran on: no host wait, and nothing changes in what runs beside what.  A call made
 * with alignments == NULL writes them to a buffer of the handle's.  The record is the bits of tts_alignment_stats on the call's
 * alignments output with n_sent taken from the ids on the host; waveform, mel, alignments and linear keep the bits of the call
 * with the setting off.  The first call after the setting was switched on is not pipelined (its buffers are new).
 * TTS_ERR_INVALID: a NULL handle. */
int tts_set_alignment_stats(tts_handle_t h, int enabled, int pad_id);
/* The records of the last tts_synthesize / tts_synthesize_host call made on the handle: stats_host, HOST [B].  Waits on the
 * host until that call's decoder and statistics have run (not for its Griffin-Lim), then copies.  TTS_ERR_INVALID: a NULL
 * pointer, a B other than that call's, or no call has been made with the setting on (the last call was made with it off). */
int tts_synth_alignment_stats(tts_handle_t h, tts_alignment_stats_t* stats_host, int B);
/* The records of a tts_synthesize_host call: they are downloaded with the waveforms (B x 56 bytes) and rotate with the three
 * buffer sets.  Waits as tts_wait_host does (same ticket rules, same reports), then hands out pinned memory of the handle,
 * valid as long as the ticket's waveform buffer.  TTS_ERR_INVALID also for a ticket whose call was made with the setting off. */
int tts_wait_host_alignment_stats(tts_handle_t h, int ticket, const tts_alignment_stats_t** stats, int* B);

/* Timing marks of synthesis: when every token of every call is spoken (tts_token_times).  A setting of the HANDLE, off by
 * default and read when a call is made; off is the call as it always was, launch for launch.  With enabled != 0,
 * tts_synthesize and tts_synthesize_host run tts_text_lengths(pad_id) on the call's device ids behind its encoder -- once: with
 * tts_set_alignment_stats on as well its lengths, and its pad_id, serve both -- and tts_token_times (n_steps[b] = p->n_steps for
 * every b, the sentence lengths read from device memory, max_jump in 1 .. 15) right behind the call's decoder and statistics, on
 * the stream the decoder ran on: no host wait, and nothing changes in what runs beside what.  A call made with alignments ==
 * NULL writes them to a buffer of the handle's.  start and the records are the bits of tts_token_times on the call's
 * alignments output with n_sent taken from the ids on the host; waveform, mel, alignments, linear and the alignment records
 * keep the bits of the call with the setting off.  The steps are the decoder's: what a step is in samples of what the call
 * delivers -- through the speaking rate, the end-of-speech cut, the output rate -- is host arithmetic (tacotron/marks.py).  The
 * first call after the setting was switched on is not pipelined (its buffers are new).  A call with Ts above
 * tts_token_times_max_tokens() is refused with TTS_ERR_UNSUPPORTED before anything is enqueued.
 * TTS_ERR_INVALID: a NULL handle; enabled with a max_jump outside 1 .. 15 (the setting stays as it was). */
int tts_set_token_times(tts_handle_t h, int enabled, int pad_id, int max_jump);
/* The results of the last tts_synthesize / tts_synthesize_host call made on the handle: start_host, HOST int32 [B][Ts + 1],
 * and stats_host, HOST [B].  Waits on the host until that call's decoder and search have run (not for its Griffin-Lim), then
 * copies on a side stream.  TTS_ERR_INVALID: a NULL pointer, a B other than that call's, or the last call was made with the
 * setting off. */
int tts_synth_token_times(tts_handle_t h, int32_t* start_host, tts_token_times_stats_t* stats_host, int B);
/* The results of a tts_synthesize_host call: they are downloaded with the waveforms (B x (4 Ts + 36) bytes) and rotate with the
 * three buffer sets.  Waits as tts_wait_host does (same ticket rules, same reports), then hands out pinned memory of the
 * handle, valid as long as the ticket's waveform buffer.  B and Ts may be NULL.  TTS_ERR_INVALID also for a ticket whose call
 * was made with the setting off. */
int tts_wait_host_token_times(tts_handle_t h, int ticket, const int32_t** start /* [B][Ts + 1] */,
                              const tts_token_times_stats_t** stats /* [B] */, int* B, int* Ts);

/* The delivery format of tts_synthesize_host: sample format and sampling rate (tts_encode, tts_resample).  A setting of the
 * HANDLE, off by default and read when a call is made.  (TTS_FMT_F32, any dither, r, r) is off: the call as it always was, launch
 * for launch and byte for byte.  Otherwise a tts_synthesize_host call runs, behind its last stage (the limiter, if that is on),
 * on the call's stream and with no host wait:
 *   rate_out != rate_in   tts_resample by rate_out / rate_in (within [0.25, 4]) of the call's rows, each over the samples it holds
 *                         (all hop (T - 1) of them, or hop (n_frames[b] - 1) with end-of-speech stopping), into rows of
 *                         N_out = tts_resampled_length(hop (T - 1), ratio) samples; row b then holds tts_resampled_length of what it
 *                         held.  The ratio's table is made before anything of the call is enqueued.
 *   format != TTS_FMT_F32 tts_encode(format, dither, seed = p->seed) of those rows over the samples they hold
 * and only the codes and the 16-byte records travel to host memory: B * N_out * tts_encode_width(format) bytes instead of the
 * float32 rows.  TTS_FMT_F32 with two rates resamples only: the bytes are float32 and there are no records.  The codes are the
 * bits of tts_encode (behind tts_resample) on the rows of the same call made with the setting off.  The resampler runs behind
 * the limiter and can overshoot its ceiling; the encoder then saturates and `clipped` counts how often: leave head room.
 * Such a call's ticket is fetched with tts_wait_host_encoded; tts_wait_host refuses it, and tts_wait_host_encoded refuses a ticket
 * of a call made with the setting off.  tts_wait_host_frames, tts_wait_host_outputs and tts_wait_host_alignment_stats are
 * unchanged.  tts_synthesize does not read the setting: its callers hold device rows and call tts_resample / tts_encode themselves.
 * The setting stays as it was on TTS_ERR_INVALID: an unknown format, an unknown dither with an encoding, rates that differ and are
 * not positive or whose ratio lies outside [0.25, 4]. */
int tts_set_output(tts_handle_t h, int format, int dither, int rate_in, int rate_out);
/* The codes of a tts_synthesize_host call made with tts_set_output on: waits as tts_wait_host does (same ticket rules, same
 * reports), then hands out pinned memory of the handle, valid as long as a ticket's waveform buffer.  data: [B][N_out] codes,
 * `bytes` of them in all; n_samples [B]: the samples each row holds (behind them: the code for zero); stats [B], NULL for
 * TTS_FMT_F32.  Every output but data may be NULL. */
int tts_wait_host_encoded(tts_handle_t h, int ticket, const void** data, size_t* bytes, int* format, int* N_out,
                          const int32_t** n_samples /* [B] held per row */, const tts_encode_stats_t** stats, int* B);

/* ---- profiling -------------------------------------------------------------------------- */
/* With option "profile"=1 the library brackets its stages with HIP events on the handle's
 * stream.  Stages: "encoder", "decoder", "postnet", "denorm", "gl_iter", "gl_final", "debug_gemm"
 * (launches of tts_debug_gemm), "eval_loss" (the loss reduction of tts_evaluate), "features" (tts_trim_bounds, the trim of tts_plan_features and
 * tts_extract_features), "speech_end" (tts_speech_frames, stand-alone or inside tts_synthesize),
 * "stretch" (tts_stretch_magnitudes / tts_stretch_rows, stand-alone or inside tts_synthesize),
 * "resample" (tts_resample, stand-alone or inside a tts_synthesize call with a pitch, and tts_resample_segments), "phase_init" (tts_phase_estimate*),
 * "mfcc" (tts_mfcc), "dtw" (tts_dtw), "f0" (tts_f0, tts_f0_compare), "loudness" (tts_loudness, tts_loudness_normalize, stand-alone
 * or inside a tts_synthesize call with a loudness target), "alignment" (tts_alignment_stats, tts_text_lengths, tts_token_times, stand-alone
 * or inside a tts_synthesize call with tts_set_alignment_stats or tts_set_token_times on), "join" (tts_join), "limiter" (tts_true_peak, tts_limit,
 * stand-alone or inside a tts_synthesize call with tts_set_limiter on), "encode" (tts_encode, stand-alone or inside a
 * tts_synthesize_host call with tts_set_output on), "warp" (tts_warp_magnitudes), "shift" (tts_shift_magnitudes), "equalize" (tts_equalize,
 * stand-alone or inside a tts_synthesize call with tts_set_equalizer on), "compress" (tts_compress, stand-alone or inside a
 * tts_synthesize call with tts_set_compressor on), "watermark" (tts_watermark_embed, tts_watermark_detect, stand-alone or the
 * embedder inside a tts_synthesize call with tts_set_watermark on), "stoi" (tts_stoi).
 * Returns accumulated milliseconds and the number of kernel launches covered since the last
 * tts_profile_reset.  Synchronises the stream. */
int tts_profile_reset(tts_handle_t h);
/* Which decoder a call of this shape takes with the handle's current options: 0 = launch per layer (decoder.hip),
 * 1 = persistent with streamed weights (decoder_persistent.hip), 2 = persistent, weight-stationary (decoder_ws.hip);
 * `pipelined` != 0: as a call under tts_synthesize's call pipeline (reserve_cus compute units), else a stand-alone call.
 * Host-only (reads the configuration; nothing is enqueued). */
int tts_decoder_kernel_choice(tts_handle_t h, int B, int T_sent, int pipelined);
/* Test hook: device pointer and size of a named internal scratch buffer of the last call
 * ("enc.bank", "enc.p1", "post.xproj", ...); contents are only valid until the next call. */
int tts_debug_workspace(tts_handle_t h, const char* name, void** dptr, size_t* bytes);
/* Host-only: the Griffin-Lim work-item cut for T frames x B utterances on n_workers compute units.
 * items[n][4] = {utterance, first frame, frames, slot word} in the order the workgroups draw them (at most max_items
 * are written); *ring_frames = frames the LDS ring of the kernel holds; returns the number of items. */
int tts_debug_gl_plan(int T, int B, int win_length, int hop_length, int n_workers, int* items, int max_items, int* ring_frames);
/* host only, as tts_debug_gl_plan: the cut of a ragged batch (n_frames[b] frames in utterance b; no run leaves its utterance) */
int tts_debug_gl_plan_ragged(const int32_t* n_frames, int B, int win_length, int hop_length, int n_workers,
                             int* items, int max_items, int* ring_frames);
/* Diagnostic: one GEMM / conv1d launch on device buffers (A [M][Cin] rows of sequences of length T, Wt [N][ktaps*Cin]). */
int tts_debug_gemm(tts_handle_t h, const float* A, const float* Wt, float* C, int M, int N, int Cin, int ktaps, int T,
                   int pool);
/* Diagnostic (needs the option "debug_hooks" = 1 on the handle): keep n_wgs workgroup slots of lds_kb KB LDS busy for ms
 * milliseconds on a private stream. */
int tts_debug_hold(tts_handle_t h, int n_wgs, int lds_kb, double ms);
int tts_profile_get(tts_handle_t h, const char* stage, float* ms_total, int64_t* launches);
/* The UUID of the handle's device as 32 hex digits + NUL (hipDeviceGetUuid) and its compute-unit count: what the
 * multi-GPU bench compares across ranks (no two ranks of one node on the same device; no reference counterpart --
 * the reference is a one-process TensorFlow session, tacotron/inference.py:44-55). */
int tts_device_info(tts_handle_t h, char uuid_hex[33], int* n_compute_units);

#ifdef __cplusplus
}
#endif
#endif /* SSTTS_HIP_H */
