// C ABI, part 2: the network's stages -- what tts_encoder_forward / tts_decoder_forward / tts_postnet_forward / tts_evaluate...
// enqueue (CBHG, the decoder forms and their choice) -- and the remaining diagnostic entry points.  The vocoder and the analysis
// side are api_griffin_lim.hip.
#include "api_internal.h"

namespace tts_api {


// CBHG (reference tacotron/layers.py:448-594) on x [B*T][c_in] -> out [B*T][2H].  Returns launches.
int run_cbhg(tts_handle_t h, const CbhgWeights& w, const char* tag, const float* x, int B, int T, float* out,
             int64_t* launches) {
    const tts_config_t& c = h->cfg;
    const int M = B * T;
    const int NB = w.n_banks, NF = w.n_filters;
    const int U = c.n_highway_units, H = c.n_gru_units;
    const std::string t(tag);
    WS(h, (t + ".bank").c_str(), float, (size_t)M * NB * NF, bank);
    WS(h, (t + ".p1").c_str(), float, (size_t)M * w.proj_filters[0], p1);
    WS(h, (t + ".p2").c_str(), float, (size_t)M * w.proj_filters[1], p2);
    WS(h, (t + ".hw0").c_str(), float, (size_t)M * U, hw0);
    WS(h, (t + ".hw1").c_str(), float, (size_t)M * U, hw1);
    WS(h, (t + ".xproj").c_str(), float, (size_t)M * 6 * H, xproj);

    // conv bank: one grouped launch, bank k writes channels [k*NF, (k+1)*NF)
    for (int k0 = 0; k0 < NB; k0 += TTS_GEMM_MAX_GROUPS) {
        GemmBatch b;
        std::memset(&b, 0, sizeof(b));
        const int ng = std::min(TTS_GEMM_MAX_GROUPS, NB - k0);
        // widest bank first: the groups are dispatched in order (blockIdx.z slowest), and a launch that ends with its
        // cheapest tiles (k = 1: 80 or 128 deep) has a shorter tail than one that ends with the k = 8 / 16 ones
        for (int i = 0; i < ng; ++i) {
            const int k = k0 + ng - 1 - i;
            b.g[i] = conv_group(x, w.c_in, k + 1, T, w.bank_wt[k], w.bank_b[k], w.bank_scale[k], w.bank_shift[k], bank,
                                NB * NF, k * NF, M, NF, ACT_RELU, 0);
        }
        HIPCHK(h, launch_gemm(h->stream, b, ng));
        ++*launches;
    }
    // projection 1: max-pool(2,1,SAME) fused into the loader, conv3 + relu + BN.  With few output tiles (the
    // encoder: 75 x 1 for 32 x 150 tokens, K = 6144) the K range is split over several workgroups per tile.
    {
        GemmGroup g = conv_group(bank, NB * NF, 3, T, w.proj_wt[0], w.proj_b[0], w.proj_scale[0], w.proj_shift[0], p1,
                                 w.proj_filters[0], 0, M, w.proj_filters[0], ACT_RELU, 1);
        const int slices = gemm_splitk_slices(g.K);
        if (slices > 1) {
            WS(h, (t + ".splitk").c_str(), float, (size_t)slices * M * g.N, part);
            HIPCHK(h, launch_gemm_splitk(h->stream, g, slices, part));
            ++*launches;
        } else {
            int rc = run_single(h, g);
            if (rc) return rc;
        }
        ++*launches;
    }
    // projection 2: conv3 + BN (linear) + residual with the CBHG input
    {
        GemmGroup g = conv_group(p1, w.proj_filters[0], 3, T, w.proj_wt[1], w.proj_b[1], w.proj_scale[1],
                                 w.proj_shift[1], p2, w.proj_filters[1], 0, M, w.proj_filters[1], ACT_NONE, 0);
        g.R = x;
        g.ldr = w.c_in;
        int rc = run_single(h, g);
        if (rc) return rc;
        ++*launches;
    }
    if (h->fused_tail && cbhg_tail_supports(w.proj_filters[1], U, H, (int)w.hw_wt.size(), M)) {
        // lifter, highway stack and the GRU input projections in one launch: the rows stay in LDS between the layers
        if (!h->tail_configured) {
            HIPCHK(h, cbhg_tail_configure());
            h->tail_configured = true;
        }
        CbhgTailParams tp;
        std::memset(&tp, 0, sizeof(tp));
        tp.X = p2; tp.ldx = w.proj_filters[1]; tp.c_in = w.proj_filters[1];
        tp.lifter_wt = w.lifter_wt; tp.lifter_b = w.lifter_b;
        tp.n_hw = (int)w.hw_wt.size();
        for (int l = 0; l < tp.n_hw; ++l) { tp.hw_wt[l] = w.hw_wt[l]; tp.hw_b[l] = w.hw_b[l]; }
        tp.gru_wt = w.gru_in_wt; tp.gru_b = w.gru_in_b;
        tp.hw_out = hw0; tp.xproj = xproj; tp.M = M;
        HIPCHK(h, launch_cbhg_tail(h->stream, tp));
        ++*launches;
    } else {
        // lifter
        {
            int rc = run_single(h, dense_group(p2, w.proj_filters[1], w.lifter_wt, w.lifter_b, hw0, U, M, U,
                                               w.proj_filters[1], ACT_RELU));
            if (rc) return rc;
            ++*launches;
        }
        // highway layers (H|T in one GEMM, gate mix in the epilogue), ping-pong buffers
        float* cur = hw0;
        float* nxt = hw1;
        for (size_t l = 0; l < w.hw_wt.size(); ++l) {
            GemmGroup g = dense_group(cur, U, w.hw_wt[l], w.hw_b[l], nxt, U, M, 2 * U, U, ACT_NONE);
            g.epi = EPI_HIGHWAY;
            int rc = run_single(h, g);
            if (rc) return rc;
            ++*launches;
            std::swap(cur, nxt);
        }
        // GRU input projections for both directions, then the recurrent kernel
        {
            int rc = run_single(h, dense_group(cur, U, w.gru_in_wt, w.gru_in_b, xproj, 6 * H, M, 6 * H, U, ACT_NONE));
            if (rc) return rc;
            ++*launches;
        }
    }
    HIPCHK(h, launch_bigru(h->stream, xproj, 6 * H, w.gru_rec, out, B, T, H, c.force_cudnn));
    ++*launches;
    return TTS_OK;
}


int check_ready(tts_handle_t h) {
    if (!h) return TTS_ERR_INVALID;
    if (!h->finalized) return fail(h, TTS_ERR_NOT_LOADED, "weights not loaded: call tts_finalize_weights first");
    return TTS_OK;
}


// ---------------------------------------------------------------------------------------- stages
// A stage entry point called by the USER (tts_synthesize orders the streams itself) runs on the main stream in the one set of
// enc.* / dec.* workspaces that the pipelined calls use on the encoder and front streams: it starts behind whatever those
// streams still hold, and the next pipelined call's encoder and decoder start behind it (serial_done, as for an unpipelined
// tts_synthesize).  Stream order alone covers the post-net (main stream on both sides).
int standalone_begin(tts_handle_t h) {
    if (!h->pl.encs) return TTS_OK;
    for (int i = 0; i < 2; ++i) {
        HIPCHK(h, h->pl.enc_ready[i].wait(h->stream));
        HIPCHK(h, h->pl.dec_done[i].wait(h->stream));
    }
    return TTS_OK;
}

int standalone_end(tts_handle_t h) {
    if (h->pl.front) HIPCHK(h, h->pl.serial_done.record(h->stream));
    return TTS_OK;
}

int encoder_impl(tts_handle_t h, const int32_t* ids, int B, int Ts, float* memory) {
    int rc = TTS_OK;
    const tts_config_t& c = h->cfg;
    const int M = B * Ts;
    WS(h, "enc.pre1", float, (size_t)M * c.enc_prenet_units[0], pre1);
    WS(h, "enc.pre2", float, (size_t)M * c.enc_prenet_units[1], pre2);
    int64_t launches = 0;
    ProfScope ps(h, ST_ENCODER, 0);
    {   // embedding lookup fused into the first pre-net GEMM (row gather)
        GemmGroup g = dense_group(h->embedding, c.embedding_size, h->enc_pre_wt[0], h->enc_pre_b[0], pre1,
                                  c.enc_prenet_units[0], M, c.enc_prenet_units[0], c.embedding_size, ACT_RELU);
        g.gather = ids;
        g.gather_rows = c.vocabulary_size;
        if ((rc = run_single(h, g))) return rc;
    }
    if ((rc = run_single(h, dense_group(pre1, c.enc_prenet_units[0], h->enc_pre_wt[1], h->enc_pre_b[1], pre2,
                                        c.enc_prenet_units[1], M, c.enc_prenet_units[1], c.enc_prenet_units[0],
                                        ACT_RELU))))
        return rc;
    launches += 2;
    if ((rc = run_cbhg(h, h->enc, "enc", pre2, B, Ts, memory, &launches))) return rc;
    if (ps.idx >= 0) h->spans[ps.idx].launches = launches;
    return TTS_OK;
}


// Which persistent decoder kernel a call of this shape takes when `budget` compute units are free for it:
// 2 = weight-stationary (decoder_ws.hip), 1 = decoder_persistent.hip, 0 = neither (launch-per-layer path).
int pd_kernel_for(tts_handle_t h, int B, int Ts, int budget) {
    const int cudnn = h->cfg.force_cudnn;
    if (h->pd_ws && decoder_ws_supports(h->dec, cudnn, B, Ts) && decoder_ws_workgroups(B) <= budget) return 2;
    if (decoder_persistent_supports(h->dec, cudnn, B, Ts) && decoder_persistent_workgroups(B) <= budget) return 1;
    return 0;
}


// ... and which one the option "persistent_decoder" picks for a call: 0 never; 2 whenever a kernel covers the configuration;
// 1 (default) by what was measured (tools/pipeline_sweep.py, tools/latency_bench.py): the weight-stationary kernel wherever it
// covers the configuration and its workgroups fit -- under the call pipeline at every batch size (round 5: 8.5 against 10.1 ms
// per call at B = 1, 9.6 against 13.7 at 32, 12.4 against 16.4 at 48: the launch-per-layer decoder's ~2000 launches queue behind
// Griffin-Lim) and, since round 6, for unpipelined calls as well: with 16 utterances per cluster (decoder_impl picks the rows)
// the loop takes 6.15-6.2 ms at B = 1 ... 64 on an idle chip against 7.5 ... 9.4 ms launch per layer and 8.25 with 32 rows
// (profiles/r06_stage_benchmarks.txt).  Its bits do not depend on the rows per cluster, on the batch size or on whether the
// call was pipelined (tests/test_gpu_persistent.py, test_gpu_full_size.py::test_shard_invariance), so a call's spectrograms no
// longer depend on the call history of the handle.  decoder_persistent.hip (streamed weights: LocalLuongAttention, or "pd_ws"
// = 0) only under the pipeline with more than 48 utterances, where the step is bound by post-net + Griffin-Lim (rounds 2-4).
int pd_choice(tts_handle_t h, int B, int Ts, int budget, bool pipelined) {
    if (h->persistent_decoder <= 0) return 0;
    const int k = pd_kernel_for(h, B, Ts, budget);
    if (h->persistent_decoder >= 2) return k;
    if (k == 2) return 2;
    if (k == 1) return (pipelined && B > 48) ? 1 : 0;
    return 0;
}


// keys = memory_layer(memory), no bias (LuongAttention, reference tacotron/model.py:205-223; the values stay the raw memory)
int attention_keys(tts_handle_t h, const float* memory, int B, int Ts, float* keys) {
    const int A = h->cfg.n_attention_units, mem = 2 * h->cfg.n_gru_units;
    return run_single(h, dense_group(memory, mem, h->mem_wt, nullptr, keys, A, B * Ts, A, mem, ACT_NONE));
}

// Which decoder a teacher-forced call takes (stand-alone, never captured): the weight-stationary kernel's teacher variant where
// the free-running call would take that kernel, else the launch-per-layer path (decoder_persistent.hip has no teacher form).
int teacher_choice(tts_handle_t h, int B, int Ts) {
    return pd_choice(h, B, Ts, h->n_cus_dev, false) == 2 && h->dec.ws_teacher ? 2 : 0;
}

// One launch of a persistent decoder: its sync words (decoder_cluster.h) from workspace `name`, laid out for `clusters` --
// a new buffer or a new layout starts with a clean sticky status word --, then what `enqueue(sync)` queues (0 or an error
// code), then the handle remembers where check_status finds the status word.
template <class Enqueue>
static int persistent_launch(tts_handle_t h, const char* name, int clusters, Enqueue enqueue) {
    WS(h, name, unsigned, dc_sync_words(clusters), sync);
    if (sync != h->pd_sync || clusters != h->pd_clusters)
        HIPCHK(h, hipMemsetAsync(dc_sync(sync, clusters).status, 0, sizeof(int), h->stream));
    if (int rc = enqueue(sync)) return rc;
    h->pd_sync = sync; h->pd_clusters = clusters; h->pd_used = true;
    return TTS_OK;
}

int decoder_impl(tts_handle_t h, const float* memory, int B, int Ts, int n_steps, float* mel, float* alignments,
                 const float* target, const StageArgs& args, std::optional<GemmGroup>* deferred) {
    int rc = TTS_OK;
    const tts_config_t& c = h->cfg;
    if (h->dec.local_d > 0 && Ts < 2 * h->dec.local_d + 1)
        return fail(h, TTS_ERR_UNSUPPORTED,
                    "LocalLuongAttention: the memory must hold at least 2*D+1 positions (for shorter inputs the reference pads "
                    "the window's 2D+1 alignments to 4D+2-T_s entries, tacotron/attention.py:294-299,85-92: its attention state "
                    "changes shape and TensorFlow fails)");
    const int A = c.n_attention_units, U = c.n_decoder_gru_units, mem = 2 * c.n_gru_units;
    const int NL = c.n_decoder_gru_layers;
    WS(h, "dec.keys", float, (size_t)B * Ts * A, keys_ws);
    // (the call pipeline computes the keys behind the encoder, on the encoder's stream, in a buffer of the call's parity)
    float* keys = args.keys ? args.keys : keys_ws;
    const bool have_keys = args.keys != nullptr;
    const size_t state_floats = (size_t)B * (A + 2 * ((size_t)A + (size_t)NL * U));   // att | h_att, h_dec[] | their second copies
    WS(h, "dec.state", float, state_floats, state);
    WS(h, "dec.tmp", float, (size_t)B * (c.dec_prenet_units[0] + c.dec_prenet_units[1] + 6 * (size_t)U), tmp);
    WS(h, "dec.ctx_parts", float, (size_t)TTS_ATT_PARTS * B * mem, ctx_parts);
    WS(h, "dec.att_stats", float, (size_t)n_steps * B * TTS_ATT_PARTS * 2, att_stats);
    // (the launch-per-layer path replays a captured graph with its buffers baked in: one y history there)
    const int pd_budget = args.cu_budget > 0 ? args.cu_budget : h->n_cus_dev;
    const int pd_kernel = target ? teacher_choice(h, B, Ts) : pd_choice(h, B, Ts, pd_budget, args.cu_budget > 0);
    const bool use_pd = pd_kernel != 0;
    const bool defer_proj = args.project_later && deferred && use_pd && !target;
    WS(h, defer_proj ? (args.parity ? "dec.yhist.odd" : "dec.yhist.even") : "dec.yhist", float, (size_t)B * n_steps * U, yhist);
    WS(h, "dec.align_raw", float, (size_t)n_steps * B * Ts, align_raw);
    DecoderScratch sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.state = state;
    sc.state_bytes = state_floats * sizeof(float);
    sc.att = state;
    sc.h_att = state + (size_t)B * A;
    for (int l = 0; l < NL; ++l) sc.h_dec[l] = state + (size_t)B * (2 * A + (size_t)l * U);
    {
        float* alt = state + (size_t)B * (2 * A + (size_t)NL * U);
        sc.h_att_alt = alt;
        for (int l = 0; l < NL; ++l) sc.h_dec_alt[l] = alt + (size_t)B * (A + (size_t)l * U);
    }
    float* t = tmp;
    sc.p1 = t; t += (size_t)B * c.dec_prenet_units[0];
    sc.p2 = t; t += (size_t)B * c.dec_prenet_units[1];
    sc.rh = t; t += (size_t)B * U;
    sc.u = t; t += (size_t)B * U;
    sc.hh = t; t += (size_t)B * U;
    sc.xi = t; t += (size_t)B * U;
    sc.y0 = t; t += (size_t)B * U;
    sc.y1 = t; t += (size_t)B * U;
    sc.ctx_parts = ctx_parts;
    sc.att_stats = att_stats;
    sc.yhist = yhist;
    sc.align_raw = align_raw;
    sc.zeros = h->zeros;
    const bool predictive = h->dec.local_d > 0 && h->dec.local_predictive;
    if (predictive) {
        WS(h, "dec.p_hist", float, (size_t)n_steps * B, p_hist);
        WS(h, "dec.err_flag", int, 4, err_flag);
        sc.p_hist = p_hist;
        sc.err_flag = err_flag;
    }

    const int OUT = c.n_mels * c.reduction;
    const int64_t per_step = 2 + 2 + 1 + 1 + 2 * NL;
    ProfScope ps(h, ST_DECODER, 3 + per_step * n_steps);
    // keys = memory_layer(memory), no bias (LuongAttention; values stay the raw memory)
    if (!have_keys && (rc = attention_keys(h, memory, B, Ts, keys))) return rc;

    if (pd_kernel == 2) {
        if (!h->ws_configured) {
            HIPCHK(h, decoder_ws_configure());
            h->ws_configured = true;
        }
        // Utterances per cluster of 16 workgroups: 16 wherever the 16 * ceil(B / 16) compute units are there for the launch --
        // every unpipelined call (the whole chip), pipelined calls of up to 2 x 16 utterances (the reserved units), and a
        // pipelined call that finds the main stream idle (the first of a burst: nothing runs beside its decoder) -- else 32.
        // The same bits either way (decoder_ws.hip), so the choice may look at the clock.
        int rows = 32;
        if (decoder_ws_workgroups(B, 16) <= pd_budget) rows = 16;
        else if (args.cu_budget > 0 && args.chip_idle && decoder_ws_workgroups(B, 16) <= h->n_cus_dev) rows = 16;
        if (h->debug_hooks && (h->pd_rows == 16 || h->pd_rows == 32) && decoder_ws_workgroups(B, h->pd_rows) <= h->n_cus_dev)
            rows = h->pd_rows;   // (tests: "pd_rows")
        const int clusters = decoder_ws_clusters(B, 16);   // layout of the sync words: that of the form with more clusters
        WS(h, "dec.ws_scratch", float, std::max(decoder_ws_scratch_floats(B, 16), decoder_ws_scratch_floats(B, 32)), ws_scratch);
        rc = persistent_launch(h, "dec.ws_sync", clusters, [&](unsigned* ws_sync) -> int {
            float* xg = nullptr;
            if (target) {   // teacher forcing: the pre-net inputs x_t W1x + b1 of all steps, one GEMM in front of the loop
                WS(h, "dec.teacher_xg", float, (size_t)B * n_steps * c.dec_prenet_units[0], xg_ws);
                HIPCHK(h, decoder_teacher_inputs(h->stream, h->dec, h->zeros, target, B, n_steps, xg_ws));
                xg = xg_ws;
            }
            HIPCHK(h, decoder_ws_enqueue(h->stream, h->dec, ws_scratch, yhist, memory, keys, B, Ts, n_steps, alignments, ws_sync,
                                         args.hold_flag, c.force_cudnn, h->debug_hooks ? h->pd_debug_delay : 0, rows, clusters, sc.p_hist,
                                         sc.err_flag, xg));
            return TTS_OK;
        });
        if (rc) return rc;
        h->pd_rows_used = rows;
    } else if (use_pd) {
        if (!h->pd_configured) {
            HIPCHK(h, decoder_persistent_configure());
            h->pd_configured = true;
        }
        rc = persistent_launch(h, "dec.pd_sync", (B + 15) / 16, [&](unsigned* pd_sync) -> int {
            HIPCHK(h, decoder_persistent_enqueue(h->stream, h->dec, sc, memory, keys, B, Ts, n_steps, alignments, pd_sync,
                                                 args.hold_flag, c.force_cudnn, h->debug_hooks ? h->pd_debug_delay : 0));
            return TTS_OK;
        });
        if (rc) return rc;
    } else if (!h->use_graph || target) {   // (a teacher-forced call is never captured)
        HIPCHK(h, decoder_enqueue(h->stream, h->dec, sc, memory, keys, B, Ts, n_steps, alignments, c.force_cudnn, target));
    } else {
        auto& k = h->dec_key;
        // (the scratch and weight structs are plain pointers and ints, zeroed before they are filled: compared bytewise)
        if (!h->dec_graph || k.memory != memory || k.keys != keys || k.align != alignments || k.B != B || k.Ts != Ts ||
            k.n_steps != n_steps || std::memcmp(&k.sc, &sc, sizeof(sc)) != 0 || std::memcmp(&k.w, &h->dec, sizeof(h->dec)) != 0) {
            if ((rc = graph_drop(h))) return rc;
            hipGraph_t graph = nullptr;
            HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            hipError_t e = decoder_enqueue(h->stream, h->dec, sc, memory, keys, B, Ts, n_steps, alignments, c.force_cudnn);
            hipError_t e2 = hipStreamEndCapture(h->stream, &graph);
            if (e != hipSuccess || e2 != hipSuccess) {
                if (graph) hipGraphDestroy(graph);
                h->err = std::string("decoder graph capture failed: ") + hipGetErrorString(e != hipSuccess ? e : e2);
                return TTS_ERR_HIP;
            }
            e = hipGraphInstantiate(&h->dec_graph, graph, nullptr, nullptr, 0);
            // (the captured graph lives as long as the executable one: see dec_graph_src)
            h->dec_graph_src = graph;
            if (e != hipSuccess) {
                hipGraphDestroy(graph);
                h->dec_graph_src = nullptr;
                h->dec_graph = nullptr;
                h->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
                return TTS_ERR_HIP;
            }
            k.memory = memory; k.keys = keys; k.align = alignments; k.B = B; k.Ts = Ts; k.n_steps = n_steps;
            k.sc = sc; k.w = h->dec;
        }
        if ((rc = graph_quiesce(h))) return rc;   // (never two launches of one executable graph in flight)
        HIPCHK(h, hipGraphLaunch(h->dec_graph, h->stream));
        HIPCHK(h, h->graph_done.record(h->stream));   // (behind the launch, outside the capture)
    }
    // OutputProjectionWrapper for all steps at once: mel[b][t][:] = y[b][t] W_o + b_o
    {
        const GemmGroup proj = dense_group(yhist, U, h->dec.out_wt, h->dec.out_b, mel, OUT, B * n_steps, OUT, U, ACT_NONE);
        if (defer_proj) {
            *deferred = proj;   // (StageArgs::project_later: the caller issues it)
        } else if ((rc = run_single(h, proj))) {
            return rc;
        }
    }
    if (predictive) {
        // a predicted window that leaves the memory: the reference fails at run time (attention.py:288-304)
        int flag = 0;
        HIPCHK(h, hipMemcpyAsync(&flag, sc.err_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (flag)
            return fail(h, TTS_ERR_UNSUPPORTED,
                        "LocalLuongAttention (predictive): a predicted attention window leaves the memory; the "
                        "reference pads such windows inconsistently and fails there too");
    }
    return TTS_OK;
}


// post-net CBHG + final Dense; with mag != null the Dense epilogue also emits the de-normalised,
// power-raised magnitude in the internal frame-major layout [B*T][FP] (fused tts_denorm_power).
int postnet_impl(tts_handle_t h, const float* mel, int B, int T, float* linear, float* mag, float ref_db,
                        float max_db, float power, int* db_flag) {
    int rc = check_ready(h);
    if (rc) return rc;
    // linear may be null when only the de-normalised magnitude is wanted (tts_synthesize without linear_out)
    if (!mel || (!linear && !mag) || B < 1 || T < 1) return fail(h, TTS_ERR_INVALID, "postnet_forward: bad arguments");
    const tts_config_t& c = h->cfg;
    const int M = B * T, H2 = 2 * c.n_gru_units, F = 1 + c.n_fft / 2;
    int64_t launches = 0;
    ProfScope ps(h, ST_POSTNET, 0);
    // apply_post_processing = 0 (reference tacotron/model.py:388-391): no CBHG, the final Dense reads the mel frames
    const float* dense_in = mel;
    int dense_k = c.n_mels;
    if (c.apply_post_processing) {
        WS(h, "post.gru", float, (size_t)M * H2, gru);
        if ((rc = run_cbhg(h, h->post, "post", mel, B, T, gru, &launches))) return rc;
        dense_in = gru;
        dense_k = H2;
    }
    GemmGroup g = dense_group(dense_in, dense_k, h->dense_wt, h->dense_b, linear, F, M, F, dense_k, ACT_NONE);
    if (mag) {
        g.C2 = mag;
        g.ldc2 = gl_fp(c.n_fft);
        g.N2 = gl_fp(c.n_fft);
        g.d_ref = ref_db;
        g.d_range = std::fabs(ref_db) + std::fabs(max_db);
        g.d_pow = power;
        g.d_flag = db_flag;
    }
    if ((rc = run_single(h, g))) return rc;
    ++launches;
    if (ps.idx >= 0) h->spans[ps.idx].launches = launches;
    return TTS_OK;
}


// What tts_evaluate and tts_teacher_forced share once their own arguments are checked: the stand-alone encoder, the decoder --
// teacher: fed from mel_target, else free-running -- and the post-net, then with a linear_target the L1 losses against the targets
// (eval_loss.hip); without one there are no losses, and no post-net either unless `linear` is asked for.  who: the entry point, for
// the messages.  Spectrograms the caller does not ask for go to workspaces of the handle.
static int evaluate_impl(tts_handle_t h, const std::string& who, bool teacher, const int32_t* ids, int B, int Ts, int n_steps,
                         const float* mel_target, const float* linear_target, float* losses, double* l1_sums, float* mel, float* alignments,
                         float* linear) {
    const tts_config_t& c = h->cfg;
    const int T = n_steps * c.reduction, F = 1 + c.n_fft / 2;
    for (const void* p : {(const void*)mel_target, (const void*)linear_target, (const void*)mel, (const void*)linear, (const void*)losses})
        if ((uintptr_t)p & 3) return fail(h, TTS_ERR_INVALID, who + ": float buffers must be 4-byte aligned");
    if (linear_target && ((uintptr_t)l1_sums & 7)) return fail(h, TTS_ERR_INVALID, who + ": l1_sums must be 8-byte aligned");
    const size_t n_mel = (size_t)B * T * c.n_mels, n_lin = (size_t)B * T * F;
    WS(h, "eval.memory", float, (size_t)B * Ts * 2 * c.n_gru_units, memory);
    float* mel_o = mel;
    if (!mel_o) {
        WS(h, "eval.mel", float, n_mel, mel_ws);
        mel_o = mel_ws;
    }
    float* lin_o = linear;
    if (!lin_o && linear_target) {
        WS(h, "eval.linear", float, n_lin, lin_ws);
        lin_o = lin_ws;
    }
    double* partial = nullptr;
    double* sums = l1_sums;
    if (linear_target) {
        WS(h, "eval.partial", double, eval_loss_partial_count(B, T, c.n_mels, F), partial_ws);
        partial = partial_ws;
        if (!sums) {
            WS(h, "eval.sums", double, (size_t)2 * B, sums_ws);
            sums = sums_ws;
        }
    }
    int rc = standalone_begin(h);
    if (rc) return rc;
    if ((rc = encoder_impl(h, ids, B, Ts, memory))) return rc;
    if ((rc = decoder_impl(h, memory, B, Ts, n_steps, mel_o, alignments, teacher ? mel_target : nullptr))) return rc;
    if (lin_o && (rc = postnet_impl(h, mel_o, B, T, lin_o, nullptr, 0.f, 0.f, 1.f))) return rc;
    if (linear_target) {
        ProfScope ps(h, ST_EVAL_LOSS, 2);
        const int blocks = 8 * std::max(1, h->n_cus_dev);   // memory-bound: 8 workgroups of 256 threads per compute unit
        HIPCHK(h, launch_eval_loss(h->stream, mel_target, mel_o, linear_target, lin_o, B, T, c.n_mels, F, blocks, partial, sums,
                                   losses));
    }
    return standalone_end(h);
}

}  // namespace tts_api

// ======================================================================================== C ABI
extern "C" {

int tts_encoder_forward(tts_handle_t h, const int32_t* ids, int B, int Ts, float* memory) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!ids || !memory || B < 1 || Ts < 1) return fail(h, TTS_ERR_INVALID, "encoder_forward: bad arguments");
    if ((rc = standalone_begin(h))) return rc;
    if ((rc = encoder_impl(h, ids, B, Ts, memory))) return rc;
    return standalone_end(h);
}

int tts_decoder_forward(tts_handle_t h, const float* memory, int B, int Ts, int n_steps, float* mel,
                        float* alignments) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!memory || !mel || B < 1 || Ts < 1 || n_steps < 1) return fail(h, TTS_ERR_INVALID, "decoder_forward: bad arguments");
    if ((rc = standalone_begin(h))) return rc;
    if ((rc = decoder_impl(h, memory, B, Ts, n_steps, mel, alignments))) return rc;
    return standalone_end(h);
}


// Teacher forcing (reference helpers.py:208-405): the decoder reads mel_target frame t*r - 1 at step t >= 1.
int tts_decoder_forward_teacher(tts_handle_t h, const float* memory, int B, int Ts, int n_steps, const float* mel_target,
                                float* mel, float* alignments) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!memory || !mel_target || !mel || B < 1 || Ts < 1 || n_steps < 1)
        return fail(h, TTS_ERR_INVALID, "decoder_forward_teacher: bad arguments");
    if ((uintptr_t)mel_target & 15) return fail(h, TTS_ERR_INVALID, "decoder_forward_teacher: mel_target must be 16-byte aligned");
    // (the target's row stride n_steps * r * n_mels is a 32-bit operand of the decoder GEMM: decoder.hip, DecGemm::lda0)
    if ((long long)n_steps * h->cfg.reduction > (1 << 24) || (long long)n_steps * h->cfg.reduction * h->cfg.n_mels > 0x7FFFFFFFll)
        return fail(h, TTS_ERR_INVALID, "decoder_forward_teacher: sizes out of range");
    if ((rc = standalone_begin(h))) return rc;
    if ((rc = decoder_impl(h, memory, B, Ts, n_steps, mel, alignments, mel_target))) return rc;
    return standalone_end(h);
}


int tts_postnet_forward(tts_handle_t h, const float* mel, int B, int T, float* linear) {
    DeviceScope dev_scope(h);
    if (!linear) return fail(h, TTS_ERR_INVALID, "postnet_forward: bad arguments");
    return postnet_impl(h, mel, B, T, linear, nullptr, 0.f, 0.f, 1.f);
}


// Mode.EVAL (reference tacotron/model.py:299-306, 432-442): the stand-alone encoder, free-running decoder and post-net of
// tts_encoder_forward / tts_decoder_forward / tts_postnet_forward (the same kernels, so the same bits), then the L1 losses
// against the targets (eval_loss.hip).  Spectrograms the caller does not ask for go to workspaces of the handle.
int tts_evaluate(tts_handle_t h, const int32_t* ids, int B, int Ts, int n_steps, const float* mel_target,
                 const float* linear_target, float* losses, double* l1_sums, float* mel, float* alignments, float* linear) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!ids || !mel_target || !linear_target || !losses || B < 1 || Ts < 1 || n_steps < 1)
        return fail(h, TTS_ERR_INVALID, "evaluate: bad arguments (ids, both targets and losses are required; B, Ts, n_steps >= 1)");
    const tts_config_t& c = h->cfg;
    const int T = n_steps * c.reduction, F = 1 + c.n_fft / 2;
    if ((long long)n_steps * c.reduction > (1 << 24) || (double)B * T * F >= 9.0e18)
        return fail(h, TTS_ERR_INVALID, "evaluate: sizes out of range");
    return evaluate_impl(h, "evaluate", false, ids, B, Ts, n_steps, mel_target, linear_target, losses, l1_sums, mel, alignments, linear);
}


// Teacher-forced forward pass (reference helpers.py:208-405 feeding the inference network): tts_evaluate with the decoder of
// tts_decoder_forward_teacher; linear_target == NULL: no losses (losses and l1_sums are then ignored).
int tts_teacher_forced(tts_handle_t h, const int32_t* ids, int B, int Ts, int n_steps, const float* mel_target,
                       const float* linear_target, float* losses, double* l1_sums, float* mel, float* alignments, float* linear) {
    DeviceScope dev_scope(h);
    int rc = check_ready(h);
    if (rc) return rc;
    if (!ids || !mel_target || (linear_target && !losses) || B < 1 || Ts < 1 || n_steps < 1)
        return fail(h, TTS_ERR_INVALID, "teacher_forced: bad arguments (ids and mel_target are required, losses with a linear "
                                        "target; B, Ts, n_steps >= 1)");
    const tts_config_t& c = h->cfg;
    const int T = n_steps * c.reduction, F = 1 + c.n_fft / 2;
    if ((long long)n_steps * c.reduction > (1 << 24) || (double)B * T * F >= 9.0e18 ||
        (long long)n_steps * c.reduction * c.n_mels > 0x7FFFFFFFll)   // (the target's row stride: tts_decoder_forward_teacher)
        return fail(h, TTS_ERR_INVALID, "teacher_forced: sizes out of range");
    if ((uintptr_t)mel_target & 15) return fail(h, TTS_ERR_INVALID, "teacher_forced: mel_target must be 16-byte aligned");
    return evaluate_impl(h, "teacher_forced", true, ids, B, Ts, n_steps, mel_target, linear_target, losses, l1_sums, mel, alignments, linear);
}


int tts_teacher_kernel_choice(tts_handle_t h, int B, int Ts) {
    if (!h || B < 1 || Ts < 1) return TTS_ERR_INVALID;
    if (!h->finalized) return fail(h, TTS_ERR_NOT_LOADED, "teacher_kernel_choice: weights not finalised");
    return teacher_choice(h, B, Ts);
}


// Diagnostic: one launch of the GEMM kernel, C[M][N] = conv(A)[M][ktaps*Cin] . Wt[N][K]^T (device pointers),
// optionally with the max-pool loader; for tools/gemm_bench.py.
int tts_debug_gemm(tts_handle_t h, const float* A, const float* Wt, float* C, int M, int N, int Cin, int ktaps, int T,
                   int pool) {
    DeviceScope dev_scope(h);
    if (!h || !A || !Wt || !C || M < 1 || N < 1 || Cin < 4 || (Cin & 3) || ktaps < 1 || T < 1 || M % T) return TTS_ERR_INVALID;
    GemmGroup g = conv_group(A, Cin, ktaps, T, Wt, nullptr, nullptr, nullptr, C, N, 0, M, N, ACT_NONE, pool);
    ProfScope ps(h, ST_DEBUG_GEMM, 1);
    const int slices = gemm_splitk_slices(g.K);   // same rule as the CBHG projections
    if (slices > 1) {
        WS(h, "debug.splitk", float, (size_t)slices * M * N, part);
        HIPCHK(h, launch_gemm_splitk(h->stream, g, slices, part));
        return TTS_OK;
    }
    return run_single(h, g);
}


// Diagnostic: occupy `n_wgs` workgroup slots of `lds_kb` KB LDS each for `ms` milliseconds on a private
// stream (to study how the other kernels behave on a partially occupied GPU).  Not part of the product path.
int tts_debug_hold(tts_handle_t h, int n_wgs, int lds_kb, double ms) {
    DeviceScope dev_scope(h);
    if (!h || n_wgs < 1 || lds_kb < 1 || lds_kb > 160) return TTS_ERR_INVALID;
    if (!h->debug_hooks) return fail(h, TTS_ERR_INVALID, "tts_debug_hold: a diagnostic; set the option \"debug_hooks\" to 1 on this handle first");
    static hipStream_t dbg = nullptr;
    static int* never = nullptr;
    static std::mutex dbg_mutex;
    std::lock_guard<std::mutex> lock(dbg_mutex);
    if (!dbg) {
        HIPCHK(h, hipStreamCreateWithFlags(&dbg, hipStreamNonBlocking));
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&never), sizeof(int)));
        HIPCHK(h, hipMemset(never, 0, sizeof(int)));
    }
    HIPCHK(h, cu_hold_configure());
    HIPCHK(h, launch_cu_hold(dbg, n_wgs, never, ms, lds_kb));
    return TTS_OK;
}

}  // extern "C"
