// C ABI, part 2b: the vocoder's and the analysis side's host code -- the tables, windows and ragged tables of Griffin-Lim, the plan
// store, the workspaces, gl_run (one GlCall, both kernel families) and what tts_griffin_lim / tts_griffin_lim_ragged / tts_stft... /
// tts_mel_spectrogram / tts_db_convert / tts_denorm_power enqueue.  Host code only: the kernels are griffin_lim.hip and
// griffin_lim_generic.hip, the argument rules and the planner gl_plan.h / gl_plan.hip.
#include "api_internal.h"

namespace tts_api {

int gl_refuse(tts_handle_t h, const GlRefusal& r) {
    return r.text.empty() ? TTS_OK : fail(h, r.unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, r.text);
}

int gl_tables(tts_handle_t h) {
    auto& g = h->gl;
    if (g.configured) return TTS_OK;
    HIPCHK(h, gl_configure());
    std::vector<float2> t1(1024), t2(1024);
    for (int k = 0; k < 1024; ++k) {
        const double a1 = -2.0 * M_PI * k / 1024.0, a2 = -2.0 * M_PI * k / 2048.0;
        t1[k] = make_float2((float)std::cos(a1), (float)std::sin(a1));
        t2[k] = make_float2((float)std::cos(a2), (float)std::sin(a2));
    }
    HIPCHK(h, hipMalloc(&g.tw1024, 1024 * sizeof(float2)));
    HIPCHK(h, hipMalloc(&g.tw2048, 1024 * sizeof(float2)));
    HIPCHK(h, hipMemcpy(g.tw1024, t1.data(), 1024 * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(g.tw2048, t2.data(), 1024 * sizeof(float2), hipMemcpyHostToDevice));
    {
        std::vector<float2> tb(1024 + 15 * 64);
        for (int k = 0; k < 1024; ++k) tb[k] = t2[k];
        for (int i = 0; i < 15 * 64; ++i) tb[1024 + i] = t1[(i & 63) * ((i >> 6) + 1)];
        HIPCHK(h, hipMalloc(&g.tables, tb.size() * sizeof(float2)));
        HIPCHK(h, hipMemcpy(g.tables, tb.data(), tb.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    g.configured = true;
    return TTS_OK;
}

int device_cus(tts_handle_t h) { return h->n_cus_dev; }   // (tts_create: the device's count, 256 where it reports none)

// periodic hann (scipy get_window('hann', win, fftbins=True)), float64 then float32
static void hann_window(int win, std::vector<double>& wd, std::vector<float>& wf) {
    wd.resize(win);
    wf.resize(win);
    for (int i = 0; i < win; ++i) {
        wd[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / win);
        wf[i] = (float)wd[i];
    }
}

// the tables of an STFT at the streaming kernel's n_fft (stft_run: every other size takes the general kernels)
static int stft_prepare(tts_handle_t h, int n, int win, int hop, int n_fft) {
    int rc = gl_refuse(h, gl_refusal("stft: ", GL_RULE_WINDOW | GL_RULE_SIGNAL | GL_RULE_ANALYSIS, n_fft, win, hop, n));
    if (rc || (rc = gl_tables(h))) return rc;
    auto& a = h->an;
    if (a.win != win) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (a.window) hipFree(a.window);
        a.window = nullptr;
        std::vector<double> wd;
        std::vector<float> wf;
        hann_window(win, wd, wf);
        HIPCHK(h, hipMalloc(&a.window, win * sizeof(float)));
        HIPCHK(h, hipMemcpy(a.window, wf.data(), win * sizeof(float), hipMemcpyHostToDevice));
        a.win = win;
    }
    return TTS_OK;
}

static int stft_run(tts_handle_t h, const float* wav, int B, int n, int n_fft, int win, int hop, float2** out, int* Tf_out) {
    const bool general = n_fft != TTS_GL_NFFT;   // the general kernels: one workgroup per frame, FFT in LDS (griffin_lim_generic.hip)
    const float2* tw = nullptr;
    int rc;
    if (general) {   // (the signal first, then the tables' rules: glg_prepare)
        if ((rc = gl_refuse(h, gl_refusal("stft: ", GL_RULE_SIGNAL | GL_RULE_ANALYSIS, n_fft, win, hop, n)))) return rc;
        if ((rc = glg_prepare(h, 0, win, hop, n_fft)) || (rc = glg_twiddles(h, n_fft, &tw))) return rc;
    } else if ((rc = stft_prepare(h, n, win, hop, n_fft))) {
        return rc;
    }
    const int Tf = 1 + n / hop, Fp = gl_fp(n_fft);   // (TTS_GL_FP at 2048)
    WS(h, "an.stft", float2, (size_t)B * Tf * Fp, buf);
    if (general) HIPCHK(h, launch_glg_stft(h->stream, wav, n, h->glg.window, tw, buf, B, Tf, Fp, n_fft, win, hop, 1, nullptr, nullptr));
    else HIPCHK(h, launch_stft(h->stream, wav, B, n, Tf, h->an.window, win, hop, h->gl.tw1024, h->gl.tw2048, buf, Fp));
    *out = buf;
    *Tf_out = Tf;
    return TTS_OK;
}

// ---- general path: any power-of-two n_fft, any window / hop (griffin_lim_generic.hip)
int gl_fp(int n_fft) { return ((n_fft / 2 + 1) + 31) & ~31; }   // padded row length (TTS_GL_FP for 2048)
// The streaming kernel is specialised to the model's configuration; everything else takes the general kernels.
bool gl_is_streaming(int n_fft, int win, int hop) { return n_fft == TTS_GL_NFFT && gl_stream_instantiated(win, hop); }

// librosa window_sumsquare (float32 buffer, sequential += of the padded squared window) as its RECIPROCAL where librosa's
// istft divides (wss > tiny(float32)), 1 elsewhere
static void recip_window_sumsquare(const std::vector<double>& wd, int n_fft, int hop, int T, std::vector<float>& wss) {
    const int win = (int)wd.size();
    const size_t n = (size_t)n_fft + (size_t)hop * (T - 1);
    wss.assign(n, 0.f);
    const int lpad = (n_fft - win) / 2;
    for (int i = 0; i < T; ++i) {
        const size_t s0 = (size_t)i * hop;
        for (int j = 0; j < win; ++j) {
            const size_t idx = s0 + lpad + j;
            if (idx < n) wss[idx] = (float)((double)wss[idx] + wd[j] * wd[j]);
        }
    }
    for (size_t i = 0; i < n; ++i) wss[i] = wss[i] > 1.17549435e-38f ? (float)(1.0 / (double)wss[i]) : 1.0f;
}

int glg_twiddles(tts_handle_t h, int n_fft, const float2** out) {
    auto& g = h->glg;
    if (!g.configured) {
        HIPCHK(h, glg_configure());
        g.configured = true;
    }
    auto it = g.tw.find(n_fft);
    if (it == g.tw.end()) {
        std::vector<float2> t(n_fft / 2);
        for (int k = 0; k < n_fft / 2; ++k) {
            const double a = -2.0 * M_PI * k / (double)n_fft;
            t[k] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        float2* d = nullptr;
        HIPCHK(h, hipMalloc(&d, t.size() * sizeof(float2)));
        HIPCHK(h, hipMemcpy(d, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice));
        it = g.tw.emplace(n_fft, d).first;
    }
    *out = it->second;
    return TTS_OK;
}

// window tables of a configuration (T = 0: the analysis side needs the window only)
int glg_prepare(tts_handle_t h, int T, int win, int hop, int n_fft) {
    if (int rc = gl_refuse(h, gl_refusal("", GL_RULE_NFFT | GL_RULE_WINDOW, n_fft, win, hop, T))) return rc;
    auto& g = h->glg;
    if (g.n_fft == n_fft && g.win == win && g.hop == hop && (T == 0 || g.T == T)) return TTS_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (g.window) hipFree(g.window);
    if (g.rwss) hipFree(g.rwss);
    g.window = g.rwss = nullptr;
    g.n_fft = 0;
    std::vector<double> wd;
    std::vector<float> wf;
    hann_window(win, wd, wf);
    HIPCHK(h, hipMalloc(&g.window, win * sizeof(float)));
    HIPCHK(h, hipMemcpy(g.window, wf.data(), win * sizeof(float), hipMemcpyHostToDevice));
    if (T > 0) {
        std::vector<float> wss;
        recip_window_sumsquare(wd, n_fft, hop, T, wss);
        HIPCHK(h, hipMalloc(&g.rwss, wss.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(g.rwss, wss.data(), wss.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    g.n_fft = n_fft; g.win = win; g.hop = hop; g.T = T;
    return TTS_OK;
}

// ---- ragged batches (tts_griffin_lim_ragged): per-utterance tables
// The first and the last E entries of recip_window_sumsquare(T) without making the n_fft + hop (T - 1) between them: entry i is a
// float32 sum, in frame order, over the frames that cover sample i, so the first E do not see frames from K on and the last E,
// counted from the end, are those of any signal of K frames or more (the same addends in the same order).  out[2 E]: [head | tail];
// a signal shorter than E has both halves start at its entry 0.
static void gl_rwss_edges(const std::vector<double>& wd, int n_fft, int hop, int T, int E, float* out) {
    const int win = (int)wd.size(), halo = (win + hop - 1) / hop - 1, lpad = (n_fft - win) / 2;
    const int K = halo + (lpad + win + hop - 1) / hop + 3;
    std::vector<float> r;
    recip_window_sumsquare(wd, n_fft, hop, std::min(T, K), r);
    const size_t m = std::min((size_t)E, r.size());
    std::fill(out, out + 2 * (size_t)E, 0.f);
    std::copy(r.begin(), r.begin() + m, out);
    std::copy(r.end() - m, r.end(), out + E);
}

int gl_rag_scratch(tts_handle_t h, int B, int T_max, int win, int hop, int n_fft, bool streaming, bool own_lens, RagScratch* s) {
    const size_t row = streaming ? 2 * (size_t)gl_rw_edge_len(n_fft, win, hop) : (size_t)n_fft + (size_t)hop * (T_max - 1);
    WS(h, "gl.rag_rw", float, (size_t)B * row, rw);
    *s = RagScratch{rw, row, nullptr};
    if (own_lens) {
        WS(h, "gl.rag_lens", int, (size_t)B, lens);
        s->lens = lens;
    }
    return TTS_OK;
}

// Uploads the lengths and the window sum-square tables of a ragged batch (h->rag.lens / rw) unless the last call's are the same.
// streaming: [B][2][E] edge tables; general kernels: a whole row of n_fft + hop (T_max - 1) per utterance, made for its length.
// d_frames: the lengths are in device memory already (tts_synthesize: what its detection kernel left, which the host has read
// and checked) -- the kernels read them there and only the tables, which the host has to compute, go up.
// The uploads are synchronous copies into ONE buffer per handle, behind a synchronisation of h->stream.  That is enough under
// the call pipeline too: the only readers of the lengths and tables are Griffin-Lim launches, and those of every call are
// enqueued on the main stream (h->stream here) -- the front and encoder streams run encoders, decoders and the phase
// initialisation of the whole padded batch, which takes no lengths.  Once the main stream is drained no reader is left.
static int gl_rag_tables(tts_handle_t h, const int32_t* n_frames, int B, int T_max, int win, int hop, int n_fft, bool streaming,
                         const int* d_frames = nullptr) {
    const int E = gl_rw_edge_len(n_fft, win, hop);
    RagScratch s;
    const int rc = gl_rag_scratch(h, B, T_max, win, hop, n_fft, streaming, !d_frames, &s);
    if (rc) return rc;
    const size_t row = s.row;
    const int* d_lens = d_frames ? d_frames : s.lens;
    std::vector<int> key = {streaming ? 1 : 0, n_fft, win, hop, T_max, B};
    key.insert(key.end(), n_frames, n_frames + B);
    auto& r = h->rag;
    if (r.lens == d_lens && r.rw == s.rw && r.tab_key == key) return TTS_OK;
    std::vector<double> wd;
    std::vector<float> wf;
    hann_window(win, wd, wf);
    std::vector<float> host((size_t)B * row, 0.f);
    std::map<int, int> first_with;   // length -> the first utterance that has it (its row is copied)
    for (int b = 0; b < B; ++b) {
        float* dst = host.data() + (size_t)b * row;
        auto it = first_with.find(n_frames[b]);
        if (it != first_with.end()) {
            std::copy(host.data() + (size_t)it->second * row, host.data() + (size_t)(it->second + 1) * row, dst);
            continue;
        }
        first_with[n_frames[b]] = b;
        if (streaming) {
            gl_rwss_edges(wd, n_fft, hop, n_frames[b], E, dst);
        } else {
            std::vector<float> full;
            recip_window_sumsquare(wd, n_fft, hop, n_frames[b], full);
            std::copy(full.begin(), full.end(), dst);
        }
    }
    r.tab_key.clear();
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (an earlier call may still read the tables)
    if (s.lens) HIPCHK(h, hipMemcpy(s.lens, n_frames, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(s.rw, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    r.lens = d_lens; r.rw = s.rw; r.tab_key = key;
    return TTS_OK;
}

void GlPlanStore::synced() {
    for (auto& e : entries) {
        e->stream = nullptr;
        e->ready.disarm();
    }
    for (void* d : retired_dev) hipFree(d);
    retired_dev.clear();
    retired_host.clear();
}

void GlPlanStore::release() {
    synced();
    for (auto& e : entries) hipFree(e->dev);
    entries.clear();
}

static bool gl_rag_all_full(const int32_t* n_frames, int B, int T) {
    for (int b = 0; b < B; ++b) if (n_frames[b] != T) return false;
    return true;
}

// the cut of p's batch (T, B, win, hop; n_frames: host lengths of a ragged batch or null) for launches of n_stage iterations on
// n_workers workgroups, from the handle's store: sets p.items / n_items / slots_per_utt / n_workers for launches on h->stream
static int gl_plan(tts_handle_t h, GlParams& p, const int32_t* n_frames, int n_workers, int n_stage, int force_runs, int force_run_len) {
    // lengths that are all equal are one length: the uniform cut and its key (gl_plan_items does the same)
    int T = p.T;
    if (n_frames && gl_rag_all_full(n_frames, p.B, n_frames[0])) {
        T = n_frames[0];
        n_frames = nullptr;
    }
    std::vector<int> key = {T, p.B, p.win, p.hop, n_workers, n_stage, force_runs, force_run_len};
    if (n_frames) key.insert(key.end(), n_frames, n_frames + p.B);
    GlPlanStore& st = h->gl_plans;
    GlPlanStore::Entry* e = nullptr;
    for (auto& q : st.entries)
        if (q->key == key) e = q.get();
    const bool found = e != nullptr;
    if (!found) {
        if ((int)st.entries.size() < GL_PLAN_CAPACITY) {
            st.entries.emplace_back(new GlPlanStore::Entry);
            e = st.entries.back().get();
        } else {   // the least recently used entry makes room
            e = st.entries.front().get();
            for (auto& q : st.entries)
                if (q->used < e->used) e = q.get();
            e->key.clear();
            if (!e->ready.done()) st.retired_host.push_back(std::move(e->items));   // (its upload may still be reading the host copy)
        }
        gl_plan_items(n_frames, T, p.B, p.win, p.hop, n_workers, n_stage, force_runs, force_run_len, &e->items, &e->slots, &e->workers);
        if (e->items.size() > e->room) {
            if (e->dev) st.retired_dev.push_back(e->dev);   // (not freed here: enqueued launches may still read it)
            e->dev = nullptr; e->room = 0; e->stream = nullptr;
            const size_t room = (e->items.size() + 255) & ~(size_t)255;
            HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&e->dev), room * sizeof(GlItem)));
            e->room = room;
        }
    }
    // From here on h->stream is where the table is used.  What another stream still holds of it comes first: the upload, for the
    // launches' sake, and the launches that read it, for the sake of an overwrite -- now (a table used again) or later.
    if (e->stream && e->stream != h->stream) {
        HIPCHK(h, e->ready.record(e->stream));
        HIPCHK(h, e->ready.wait(h->stream));
    }
    if (!found) {
        HIPCHK(h, hipMemcpyAsync(e->dev, e->items.data(), e->items.size() * sizeof(GlItem), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, e->ready.record(h->stream));
        e->key = std::move(key);
    }
    e->stream = h->stream;
    e->used = ++st.clock;
    p.items = e->dev;
    p.n_items = (int)e->items.size();
    p.slots_per_utt = e->slots;
    p.n_workers = e->workers;
    return TTS_OK;
}

// fast Griffin-Lim keeps the previous projection per bin for a call that has a second iteration to use it
static bool gl_momentum_on(int momentum, int n_iter) { return momentum > 0 && n_iter > 1; }

int glg_scratch(tts_handle_t h, int B, int T, int win, int n_fft, int momentum, int n_iter, GlgScratch* s) {
    const int Fp = gl_fp(n_fft);
    WS(h, "glg.phase", float2, (size_t)B * T * Fp, ph);
    WS(h, "glg.frames", float, (size_t)B * T * win, frames);
    WS(h, "glg.mse_partial", float, (size_t)B * T, msep);
    *s = GlgScratch{ph, frames, msep, nullptr, false};
    if (gl_momentum_on(momentum, n_iter)) {
        const unsigned allocs = h->ws_allocs;
        WS(h, "glg.mom", float2, (size_t)B * T * Fp, mc);
        s->mom = mc;
        s->mom_grew = h->ws_allocs != allocs;
    }
    return TTS_OK;
}

// The error of a call's last iteration from its partial sums -- `chunks` per utterance; per_frame: one per frame, of which a ragged
// utterance's own count -- or 0 for a call without iterations.  d_lens: the device lengths of a ragged batch, or null.
static int gl_error(tts_handle_t h, const GlCall& c, const float* partial, int chunks, bool per_frame, const int* d_lens) {
    const int F = 1 + c.n_fft / 2;
    if (c.n_iter > 0 && d_lens) HIPCHK(h, launch_gl_mse_reduce_ragged(h->stream, partial, c.B, chunks, F, d_lens, per_frame ? 1 : 0, c.mse));
    else if (c.n_iter > 0) HIPCHK(h, launch_gl_mse_reduce(h->stream, partial, c.B, chunks, (float)((double)F * c.T), c.mse));
    else HIPCHK(h, hipMemsetAsync(c.mse, 0, c.B * sizeof(float), h->stream));
    return TTS_OK;
}

// The general kernels' family of gl_run: c.mag is [B][T][Fp] (Fp = gl_fp(n_fft))
static int gl_run_general(tts_handle_t h, const GlCall& c) {
    const int B = c.B, T = c.T, win = c.win, hop = c.hop, n_fft = c.n_fft;
    int rc = gl_refuse(h, gl_refusal("griffin_lim: ", GL_RULE_FRAMES | GL_RULE_SIGNAL, n_fft, win, hop, T));
    if (rc || (rc = glg_prepare(h, T, win, hop, n_fft))) return rc;
    // a ragged batch: the kernels take the lengths and a row of 1 / window sum-square per utterance (made for its length)
    const int* d_lens = nullptr;
    const float* rwss = h->glg.rwss;
    if (c.n_frames) {
        if ((rc = gl_rag_tables(h, c.n_frames, B, T, win, hop, n_fft, false, c.d_frames))) return rc;
        d_lens = h->rag.lens;
        rwss = h->rag.rw;
    }
    const float2* tw = nullptr;
    if ((rc = glg_twiddles(h, n_fft, &tw))) return rc;
    const int F = 1 + n_fft / 2, Fp = gl_fp(n_fft), L = hop * (T - 1);
    GlgScratch g;
    if ((rc = glg_scratch(h, B, T, win, n_fft, c.momentum, c.n_iter, &g))) return rc;
    float2 *const ph = g.phase, *const mom_c = g.mom;   // (fast Griffin-Lim: the previous projection per bin, or null)
    float *const frames = g.frames, *const msep = g.mse_partial;
    const float alpha = (float)(c.momentum / 1000.0);
    float* sig = c.wav;   // every iteration's signal estimate lives in the caller's buffer: the last one is the result
    HIPCHK(h, launch_glg_phase_init(h->stream, c.init_ft, c.seed, ph, B, F, T, Fp, d_lens));
    {
        ProfScope ps(h, ST_GL_ITER, 3 * (int64_t)c.n_iter);
        for (int it = 0; it < c.n_iter; ++it) {
            HIPCHK(h, launch_glg_istft(h->stream, c.mag, ph, h->glg.window, rwss, tw, frames, sig, B, T, Fp, n_fft, win, hop, d_lens));
            const bool want_mse = c.mse && it == c.n_iter - 1;
            HIPCHK(h, launch_glg_stft(h->stream, sig, L, h->glg.window, tw, ph, B, T, Fp, n_fft, win, hop, 0, c.mag,
                                      want_mse ? msep : nullptr, mom_c, alpha, it == 0, d_lens));
        }
    }
    if (c.mse && (rc = gl_error(h, c, msep, T, true, d_lens))) return rc;
    {
        ProfScope ps(h, ST_GL_FINAL, 2);
        HIPCHK(h, launch_glg_istft(h->stream, c.mag, ph, h->glg.window, rwss, tw, frames, c.wav, B, T, Fp, n_fft, win, hop, d_lens));
    }
    // (a ragged batch: the tail of a row is 0 -- glg_istft writes it -- and stays 0; the peak is the utterance's own)
    if (c.peak_normalize) HIPCHK(h, launch_peak_normalize(h->stream, c.wav, B, L));
    return TTS_OK;
}

int gl_prepare(tts_handle_t h, int T, int win, int hop, int n_fft) {
    if (!gl_is_streaming(n_fft, win, hop)) return fail(h, TTS_ERR_UNSUPPORTED, "griffin_lim: the streaming kernel is instantiated for 1102 / 275 and 800 / 200 at n_fft 2048 only");
    // (an instantiated pair: its window and hop are legal and ceil(window / hop) is 4 or 5 of the kernel's 8 -- what is left is T and the signal)
    int rc = gl_refuse(h, gl_refusal("griffin_lim: ", GL_RULE_WINDOW | GL_RULE_FRAMES | GL_RULE_SIGNAL, n_fft, win, hop, T));
    if (rc || (rc = gl_tables(h))) return rc;
    auto& g = h->gl;
    if (g.win == win && g.hop == hop && g.T == T) return TTS_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (g.window) hipFree(g.window);
    if (g.wss) hipFree(g.wss);
    if (g.wlane) hipFree(g.wlane);
    g.window = g.wss = g.wlane = nullptr;
    std::vector<double> wd;
    std::vector<float> wf, wss;
    hann_window(win, wd, wf);
    recip_window_sumsquare(wd, n_fft, hop, T, wss);   // (the kernels multiply where librosa's istft divides)
    HIPCHK(h, hipMalloc(&g.window, win * sizeof(float)));
    HIPCHK(h, hipMalloc(&g.wss, wss.size() * sizeof(float)));
    HIPCHK(h, hipMemcpy(g.window, wf.data(), win * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(g.wss, wss.data(), wss.size() * sizeof(float), hipMemcpyHostToDevice));
    {
        std::vector<float> wl(2 * 16 * 2 * 64);
        gl_build_wlane(wf.data(), wss.data(), win, hop, T, wl.data());
        HIPCHK(h, hipMalloc(&g.wlane, wl.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(g.wlane, wl.data(), wl.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    g.win = win; g.hop = hop; g.T = T;
    return TTS_OK;
}

int gl_scratch(tts_handle_t h, int B, int T, int momentum, int n_iter, bool frame_mse, int min_slots, bool own_phase, GlScratch* s) {
    const int FP = TTS_GL_FP;
    *s = GlScratch{};
    if (gl_momentum_on(momentum, n_iter)) {   // the previous projection per bin, 8 bytes
        const unsigned allocs = h->ws_allocs;
        WS(h, "gl.mom", float2, (size_t)B * T * FP, mc);
        s->mom = mc;
        s->mom_grew = h->ws_allocs != allocs;
    }
    // (with momentum the squared error is kept per frame: gl_stream_kernel, MOM)
    const int slots = std::max(min_slots, T / (GL_NW / 2) + 1);
    WS(h, "gl.mse_partial", float, (size_t)B * ((s->mom && frame_mse) ? std::max(slots, T) : slots), msep);
    WS(h, "gl.counter_ring", unsigned, GL_RING, ring);
    s->mse_partial = msep; s->counter_ring = ring;
    if (own_phase) {   // 4 bytes per bin: the state between iterations is a 32-bit phasor code (griffin_lim.hip)
        WS(h, "gl.phase0", unsigned, (size_t)B * T * FP * (gl_state_bytes() / sizeof(unsigned)), own0);
        WS(h, "gl.phase1", unsigned, (size_t)B * T * FP * (gl_state_bytes() / sizeof(unsigned)), own1);
        s->phase[0] = reinterpret_cast<float2*>(own0); s->phase[1] = reinterpret_cast<float2*>(own1);
    }
    return TTS_OK;
}

// ---- the streaming kernel's family of gl_run, step by step over the call and this state.  c.mag is [B][T][TTS_GL_FP].
struct GlStream {
    GlParams p, pw;          // the launches' arguments under the narrow cut, and under the wide one: a second cut of the same frames
    int n_cus, free_cus;     // workgroups of a wide and of a narrow launch
    int per_launch;          // iterations per launch the cuts are made for
    bool two_cuts, wide_planned;
    float* msep;
    float2 *cur, *nxt;       // the phasor codes an iteration reads and writes
    int launch_idx = 0, mse_chunks = 0;
};

// Iterations per launch: gl_pair (1, 2 or 3; default in the handle) as far as the LDS ring holds that many stages.  Fast Griffin-Lim
// (option "gl_momentum"): a call that has a second iteration to use the previous projection runs one iteration per launch
// (gl_stream_kernel, MOM) and is cut for that form.
static int gl_iters_per_launch(int gl_pair, int win, int hop, int momentum, int n_iter) {
    int n = gl_pair < 1 ? 1 : (gl_pair > 3 ? 3 : gl_pair);
    while (n > 1 && gl_stream_ring_frames(win, hop, n) <= 0) --n;
    return gl_momentum_on(momentum, n_iter) ? 1 : n;
}

// Step 1: the tables and the launch arguments every launch of the call shares
static int gl_stream_params(tts_handle_t h, const GlCall& c, GlStream& s) {
    const int n_fft = c.n_fft, win = c.win, hop = c.hop;
    int rc = gl_prepare(h, c.T, win, hop, n_fft);
    if (rc) return rc;
    // a ragged batch (T is T_max): the lengths and every utterance's own window sum-square ends, on the device.  Under the
    // call pipeline as well: both cuts are made for the lengths, the phasor codes of the caller's pair cover the whole padded
    // batch (written on the front stream without lengths: a superset of what the ragged launches read)
    if (c.n_frames && (rc = gl_rag_tables(h, c.n_frames, c.B, c.T, win, hop, n_fft, true, c.d_frames))) return rc;
    GlParams& p = s.p;
    std::memset(&p, 0, sizeof(p));
    p.mag = c.mag;
    p.window = h->gl.window; p.rwss = h->gl.wss; p.wlane = h->gl.wlane;
    p.tw1024 = h->gl.tw1024; p.tw2048 = h->gl.tw2048; p.tables = h->gl.tables;
    p.B = c.B; p.T = c.T; p.FP = TTS_GL_FP; p.win = win; p.hop = hop;
    p.ncol = (win + hop - 1) / hop;
    p.F = 1 + n_fft / 2; p.seed = c.seed;
    if (c.n_frames) {   // (launch_gl_stream then takes the RAG instantiations)
        p.n_frames = h->rag.lens;
        p.rw_edge = h->rag.rw;
        p.rw_E = gl_rw_edge_len(n_fft, win, hop);
    }
    return TTS_OK;   // (an instantiated pair fits the LDS ring: gl_stream_ring_frames >= 1)
}

// Step 2: the cuts.  The narrow one, for the workgroups that really run side by side, and -- c.wide_from >= 0, the pipelined
// tts_synthesize, see gl_wide_from there -- the wide one for the launches from that index on, cut for ALL compute units: the
// second stream's decoder has left its share by then.
static int gl_stream_cuts(tts_handle_t h, const GlCall& c, GlStream& s) {
    s.n_cus = (h->debug_hooks && h->gl_workers >= 16 && h->gl_workers <= device_cus(h)) ? h->gl_workers : device_cus(h);   // (tools: "gl_workers")
    // the pipelined tts_synthesize keeps `reserve_cus` compute units free of Griffin-Lim for its second stream
    const int held = (c.under_reservation && h->reserve_cus > 0) ? h->reserve_cus : 0;
    s.per_launch = gl_iters_per_launch(h->gl_pair, c.win, c.hop, c.momentum, c.n_iter);
    // (without momentum nothing differs from what it was: p.mom_c stays null and the plain instantiations are launched)
    if (gl_momentum_on(c.momentum, c.n_iter)) s.p.mom_alpha = (float)(c.momentum / 1000.0);
    // (the cut decides who does which frames, never the waveform's bits: every sample is summed over the frames that cover it in
    //  ascending order whatever run they lie in -- tests/test_gpu_audio.py::test_griffin_lim_bits_do_not_depend_on_the_cut)
    s.free_cus = s.n_cus - held > 16 ? s.n_cus - held : s.n_cus;
    int rc = gl_plan(h, s.p, c.n_frames, s.free_cus, s.per_launch, h->debug_hooks ? h->gl_runs : 0, h->debug_hooks ? h->gl_run_len : 0);
    if (rc) return rc;
    s.pw = s.p;
    s.two_cuts = held > 0 && c.wide_from >= 0 && s.n_cus - held > 16 && !(h->debug_hooks && (h->gl_runs || h->gl_run_len));
    // A ragged batch under the pipeline (tts_synthesize with end-of-speech stopping) has new lengths in every call, so both
    // cuts are planned in the call -- on the host, behind the wait for the lengths, while the main stream is idle.  Its wide
    // cut is therefore planned where its first launch comes up (gl_stream_cut): the narrow launches are enqueued by then and
    // the planner runs beside them.  (The partials' workspace is sized for any planned cut: gl_scratch.)
    s.wide_planned = !(s.two_cuts && c.n_frames);
    if (s.two_cuts && s.wide_planned) rc = gl_plan(h, s.pw, c.n_frames, s.n_cus, s.per_launch, 0, 0);
    return rc;
}

// The launch arguments of launch `s.launch_idx`, and its grid: the narrow cut's, or from c.wide_from on the wide one's
static int gl_stream_cut(tts_handle_t h, const GlCall& c, GlStream& s, GlParams** q, int* grid) {
    const bool wide = s.two_cuts && s.launch_idx >= c.wide_from;
    if (wide && !s.wide_planned) {
        s.wide_planned = true;
        if (int rc = gl_plan(h, s.pw, c.n_frames, s.n_cus, s.per_launch, 0, 0)) return rc;
    }
    *q = wide ? &s.pw : &s.p;
    // no more workgroups than the plan counts on: one that finds its compute unit taken (the call pipeline's other
    // stream) would start when the first of the others leaves, load its tables, find no item and only
    // lengthen the launch
    *grid = wide ? s.n_cus : s.free_cus;
    return TTS_OK;
}

// One zeroed work counter per launch (the persistent workgroups draw their item ids from it): slots of a ring that is
// zeroed ONCE; a launch takes the next slot and zeroes the slot of the launch before it on the stream, which is drained
// by then.  (Until round 4 a memset per call: two fill kernels and their dependencies, 0.1 ms between the post-net and
// the first Griffin-Lim launch of every call, on the stream that bounds the step.)
hipError_t GlCounterRing::start(unsigned* buf, hipStream_t on) {
    if (buf == ring && on == stream) return hipSuccess;
    const hipError_t e = hipMemsetAsync(buf, 0, GL_RING * sizeof(unsigned), on);   // new buffer, or launches of another stream before these
    if (e == hipSuccess) { ring = buf; stream = on; last = nullptr; }
    return e;
}

void GlCounterRing::next(GlParams& q) {
    q.clear_counter = last;
    q.work_counter = last = ring + (seq++ % GL_RING);
}

// Step 3: the workspaces, the counters and the initial phasor codes
static int gl_stream_begin(tts_handle_t h, const GlCall& c, GlStream& s) {
    // (a pipelined call finds these as synth_workspaces left them, asked for the same shape; the slots of the cuts in hand count
    //  only where a forced cut has more runs than any planned one)
    GlScratch ws;
    int rc = gl_scratch(h, c.B, c.T, c.momentum, c.n_iter, c.mse != nullptr, std::max(s.p.slots_per_utt, s.pw.slots_per_utt), !c.phase_pair, &ws);
    if (rc) return rc;
    s.p.mom_c = s.pw.mom_c = ws.mom;
    s.msep = ws.mse_partial;
    s.cur = c.phase_pair ? c.phase_pair[0] : ws.phase[0];
    s.nxt = c.phase_pair ? c.phase_pair[1] : ws.phase[1];
    HIPCHK(h, h->gl_ring.start(ws.counter_ring, h->stream));
    // a seeded start with at least one iteration needs no codes: the first launch makes the initial phasors itself
    if (!c.phase_ready && !(!c.init_ft && c.n_iter >= 1))
        HIPCHK(h, launch_phase_init(h->stream, c.init_ft, c.seed, s.cur, c.B, s.p.F, c.T, TTS_GL_FP, s.p.n_frames));
    return TTS_OK;
}

// Step 4: the iterations.  The streaming kernel runs up to s.per_launch iterations per launch (gl_stream_kernel, NST) wherever no
// per-iteration result is asked for: all of them, or all but the last (the mse is the last iteration's)
static int gl_stream_iterate(tts_handle_t h, const GlCall& c, GlStream& s) {
    ProfScope ps(h, ST_GL_ITER, c.n_iter);
    s.mse_chunks = s.p.slots_per_utt;
    for (int it = 0; it < c.n_iter; ++s.launch_idx) {
        const bool want_mse = c.mse && it == c.n_iter - 1;
        const int left = c.n_iter - (c.mse ? 1 : 0) - it;   // iterations that may share a launch
        const int n_stage = left >= s.per_launch ? s.per_launch : (left >= 1 ? left : 1);
        GlParams* q;
        int grid;
        if (int rc = gl_stream_cut(h, c, s, &q, &grid)) return rc;
        q->phase_in = s.cur;
        q->phase_out = s.nxt;
        q->seeded = !c.init_ft && it == 0;
        q->mom_first = it == 0;
        q->mse_partial = want_mse ? s.msep : nullptr;
        if (want_mse) s.mse_chunks = q->mom_c ? c.T : q->slots_per_utt;
        h->gl_ring.next(*q);
        HIPCHK(h, launch_gl_stream(h->stream, *q, grid, 0, n_stage));
        std::swap(s.cur, s.nxt);
        it += n_stage;
    }
    return TTS_OK;
}

// Step 5: the final launch -- the waveform and, for a call that is peak-normalised, every run's peak -- and the scaling
static int gl_stream_final(tts_handle_t h, const GlCall& c, GlStream& s) {
    const size_t L = (size_t)c.hop * (c.T - 1);
    int peak_chunks;
    {
        ProfScope ps(h, ST_GL_FINAL, 1);
        GlParams* q;
        int grid;
        if (int rc = gl_stream_cut(h, c, s, &q, &grid)) return rc;
        q->seeded = 0;
        q->phase_in = s.cur;
        q->phase_out = nullptr;
        q->mse_partial = nullptr;
        q->wav = c.wav;
        q->peak_partial = c.peak_normalize ? s.msep : nullptr;   // the mse partials are consumed by now
        // a ragged batch: what lies behind an utterance's end in its row is 0 (one fill; the launch writes the signals over it)
        if (c.n_frames && !gl_rag_all_full(c.n_frames, c.B, c.T)) HIPCHK(h, hipMemsetAsync(c.wav, 0, c.B * L * sizeof(float), h->stream));
        h->gl_ring.next(*q);
        HIPCHK(h, launch_gl_stream(h->stream, *q, grid, 1, 1));
        peak_chunks = q->slots_per_utt;
    }
    // (dividing by the peak inside the final launch -- by the workgroup that finishes an utterance's last run -- was built
    //  and measured: +0.09 ms on that launch against the 0.05 ms of this kernel)
    // (a ragged batch: an utterance's runs hold the peak of its own hop (n_frames[b] - 1) samples -- fmaxf, so a NaN sample takes
    //  no part, as in tts_peak_normalize; the zero tail of the row is divided like the rest and stays 0)
    if (c.peak_normalize) HIPCHK(h, launch_peak_scale(h->stream, c.wav, c.B, (int)L, s.msep, peak_chunks));
    return TTS_OK;
}

static int gl_run_streaming(tts_handle_t h, const GlCall& c) {
    GlStream s;
    int rc;
    if ((rc = gl_stream_params(h, c, s)) || (rc = gl_stream_cuts(h, c, s)) || (rc = gl_stream_begin(h, c, s)) || (rc = gl_stream_iterate(h, c, s))) return rc;
    if (c.mse && (rc = gl_error(h, c, s.msep, s.mse_chunks, s.p.mom_c != nullptr, s.p.n_frames))) return rc;
    return gl_stream_final(h, c, s);
}

int gl_run(tts_handle_t h, const GlCall& c) { return gl_is_streaming(c.n_fft, c.win, c.hop) ? gl_run_streaming(h, c) : gl_run_general(h, c); }

// The init_phase of a Griffin-Lim call.  An explicit one always wins; otherwise, with gl_init (the option "gl_init" = 1), the phases are
// estimated from the magnitudes the call reconstructs from (time-major rows, `magi`) into a workspace in the public layout and
// handed on exactly as a caller's array would be -- the launches cannot tell the two apart, so the waveform has the same bits.
int gl_init_phase(tts_handle_t h, int gl_init, const float* magi, const float* init_phase, int B, int T, int row_stride, const int32_t* n_frames,
                  int n_fft, int hop, const float** out) {
    *out = init_phase;
    if (init_phase || !gl_init) return TTS_OK;
    PhaseScratch s;
    int rc = phase_estimate_scratch(h, B, T, n_fft, false, true, &s);
    if (rc || (rc = phase_estimate_impl(h, magi, B, T, row_stride, true, n_frames, n_fft, hop, s.init_est))) return rc;
    *out = s.init_est;
    return TTS_OK;
}

// The time-major magnitudes Griffin-Lim reconstructs from: B utterances of T rows of row_stride floats.
int gl_mag_scratch(tts_handle_t h, int B, int T, int row_stride, float** mag) {
    WS(h, "gl.mag", float, (size_t)B * T * row_stride, m);
    *mag = m;
    return TTS_OK;
}

// reference audio/conversion.py:47-49: decibel_to_magnitude raises AssertionError when some dB value is below
// -100.  The lowest value inv_normalize_decibel can produce is ref - (|ref| + |max|) (clip(x) == 0): with the
// reference's constants (6.02, 99.89) that is -93.87 dB, so the assertion cannot fire and nothing is checked.
// Constants that allow it get the data-dependent check the reference makes: the de-normalising kernels raise
// a device flag, which the caller reads back (one stream synchronisation, only in that configuration).  tts_db_convert's
// dB-to-magnitude mode arms and reads the same flag around its own kernel, whatever the constants.
bool denorm_can_assert(float ref_db, float max_db) {
    return ref_db - (std::fabs(ref_db) + std::fabs(max_db)) < -100.0f;
}

int denorm_flag_arm(tts_handle_t h, int** flag) {
    if (!h->an.flag) HIPCHK(h, hipMalloc(&h->an.flag, sizeof(int)));
    HIPCHK(h, hipMemsetAsync(h->an.flag, 0, sizeof(int), h->stream));
    *flag = h->an.flag;
    return TTS_OK;
}

int denorm_flag_read(tts_handle_t h) {
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->an.flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag)
        return fail(h, TTS_ERR_DB_RANGE,
                    "\"conversion.decibel_to_magnitude\" was asked to convert a dB value smaller -100 dB.");
    return TTS_OK;
}

// tts_griffin_lim (n_frames null) and tts_griffin_lim_ragged (T is T_max) under the name `who`: the check, the transposed magnitudes,
// the initial phase and gl_run.  The rules answer as "griffin_lim", a ragged batch's lengths under the entry point's own name.
static int griffin_lim_entry(tts_handle_t h, const std::string& who, const float* mag, const float* init_phase, uint64_t seed, int B, int T,
                             const int32_t* n_frames, int n_iter, int win, int hop, int n_fft, float* wav, float* mse) {
    if (!h || !mag || !wav || B < 1 || n_iter < 0) return fail(h, TTS_ERR_INVALID, who + ": bad arguments");
    // every length is checked before anything is enqueued.  (The streaming kernel's n_fft is 2048: nothing to ask.)
    const bool streaming = gl_is_streaming(n_fft, win, hop);
    int rc = gl_refuse(h, gl_refusal("griffin_lim: ", (streaming ? 0 : GL_RULE_NFFT) | GL_RULE_WINDOW | GL_RULE_FRAMES, n_fft, win, hop, T));
    if (rc || (n_frames && (rc = gl_refuse(h, gl_refusal(who + ": ", 0, n_fft, win, hop, T, n_frames, B))))) return rc;
    // (the general kernels answer a signal of one length that is too short in gl_run, behind the transpose)
    if (streaming && (rc = gl_prepare(h, T, win, hop, n_fft))) return rc;
    // the lengths go to the device first: the transpose, too, stops at n_frames[b] (no padding column is read by any kernel)
    if (n_frames && (rc = gl_rag_tables(h, n_frames, B, T, win, hop, n_fft, streaming))) return rc;
    const int F = 1 + n_fft / 2, Fp = gl_fp(n_fft);
    float* magi = nullptr;
    if ((rc = gl_mag_scratch(h, B, T, Fp, &magi))) return rc;
    HIPCHK(h, launch_mag_ft_to_tf(h->stream, mag, magi, B, F, T, Fp, n_frames ? h->rag.lens : nullptr));
    // (the stand-alone calls have no copy of the settings: they read the handle's start and momentum here)
    if ((rc = gl_init_phase(h, h->settings.gl_init, magi, init_phase, B, T, Fp, n_frames, n_fft, hop, &init_phase))) return rc;
    GlCall c;
    c.mag = magi; c.init_ft = init_phase; c.seed = seed;
    c.B = B; c.T = T; c.n_iter = n_iter; c.win = win; c.hop = hop; c.n_fft = n_fft;
    c.wav = wav; c.mse = mse;
    c.n_frames = n_frames;
    c.momentum = h->settings.gl_momentum;
    return gl_run(h, c);
}

}  // namespace tts_api

// ======================================================================================== C ABI
extern "C" {

int tts_denorm_power(tts_handle_t h, const float* linear, int B, int T, int F, float ref_db, float max_db, float power,
                     float* mag) {
    DeviceScope dev_scope(h);
    if (!h || !linear || !mag || B < 1 || T < 1 || F < 1) return fail(h, TTS_ERR_INVALID, "denorm_power: bad arguments");
    int rc;
    int* flag = nullptr;
    if (denorm_can_assert(ref_db, max_db) && (rc = denorm_flag_arm(h, &flag))) return rc;
    const int FP = (F + 3) & ~3;
    WS(h, "denorm.tmp", float, (size_t)B * T * FP, tmp);
    {
        ProfScope ps(h, ST_DENORM, 2);
        HIPCHK(h, launch_denorm_power(h->stream, linear, tmp, (size_t)B * T, F, FP, ref_db, max_db, power, flag));
        HIPCHK(h, launch_tf_to_ft(h->stream, tmp, mag, B, F, T, FP));
    }
    return flag ? denorm_flag_read(h) : TTS_OK;
}

int tts_griffin_lim(tts_handle_t h, const float* mag, const float* init_phase, uint64_t seed, int B, int T, int n_iter,
                    int win_length, int hop_length, int n_fft, float* wav, float* mse) {
    DeviceScope dev_scope(h);
    return griffin_lim_entry(h, "griffin_lim", mag, init_phase, seed, B, T, nullptr, n_iter, win_length, hop_length, n_fft, wav, mse);
}

// tts_griffin_lim for utterances of different lengths in one padded batch (include/sstts_hip.h)
int tts_griffin_lim_ragged(tts_handle_t h, const float* mag, const float* init_phase, uint64_t seed, int B, int T_max,
                           const int32_t* n_frames, int n_iter, int win_length, int hop_length, int n_fft, float* wav, float* mse) {
    DeviceScope dev_scope(h);
    if (!n_frames) return fail(h, TTS_ERR_INVALID, "griffin_lim_ragged: bad arguments");
    return griffin_lim_entry(h, "griffin_lim_ragged", mag, init_phase, seed, B, T_max, n_frames, n_iter, win_length, hop_length, n_fft, wav, mse);
}

int tts_peak_normalize(tts_handle_t h, float* wav, int B, int n) {
    DeviceScope dev_scope(h);
    if (!h || !wav || B < 1 || n < 1) return fail(h, TTS_ERR_INVALID, "peak_normalize: bad arguments");
    HIPCHK(h, launch_peak_normalize(h->stream, wav, B, n));
    return TTS_OK;
}

// tts_stft (mode 0: the complex spectrum) and tts_stft_magnitude (mode 1: |S| ^ power) under the name `who`
static int stft_entry(tts_handle_t h, const char* who, const float* wav, int B, int n, int n_fft, int win, int hop, int mode, float power, float* out) {
    DeviceScope dev_scope(h);
    if (!h || !wav || !out || B < 1) return fail(h, TTS_ERR_INVALID, std::string(who) + ": bad arguments");
    float2* buf;
    int Tf;
    int rc = stft_run(h, wav, B, n, n_fft, win, hop, &buf, &Tf);
    if (rc) return rc;
    HIPCHK(h, launch_cplx_tf_to_ft(h->stream, buf, out, B, 1 + n_fft / 2, Tf, gl_fp(n_fft), mode, power));
    return TTS_OK;
}

int tts_stft(tts_handle_t h, const float* wav, int B, int n, int n_fft, int win_length, int hop_length, float* out) {
    return stft_entry(h, "stft", wav, B, n, n_fft, win_length, hop_length, 0, 1.0f, out);
}

int tts_stft_magnitude(tts_handle_t h, const float* wav, int B, int n, int n_fft, int win_length, int hop_length,
                       float power, float* lin) {
    return stft_entry(h, "stft_magnitude", wav, B, n, n_fft, win_length, hop_length, 1, power, lin);
}

int tts_mel_spectrogram(tts_handle_t h, const float* lin, int B, int n_frames, int n_fft, int sr, int n_mels, float fmin,
                        float fmax, float* mel) {
    DeviceScope dev_scope(h);
    if (!h || !lin || !mel || B < 1 || n_frames < 1 || n_mels < 1 || sr < 1)
        return fail(h, TTS_ERR_INVALID, "mel_spectrogram: bad arguments");
    if (n_fft < 2 || (n_fft & 1)) return fail(h, TTS_ERR_INVALID, "mel_spectrogram: n_fft must be even");
    const int F = 1 + n_fft / 2, FP = gl_fp(n_fft);
    auto& a = h->an;
    if (!a.mel_wt || a.sr != sr || a.n_fft != n_fft || a.n_mels != n_mels || a.fmin != fmin || a.fmax != fmax) {
        // librosa.filters.mel(htk=True, norm=1) [librosa-0.6]; reference audio/features.py:75-80
        auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
        auto mel2hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
        const double fmx = fmax > 0 ? fmax : sr / 2.0;
        std::vector<double> mel_f(n_mels + 2);
        const double m0 = hz2mel(fmin), m1 = hz2mel(fmx);
        for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel2hz(m0 + (m1 - m0) * i / (n_mels + 1));
        std::vector<float> wt((size_t)n_mels * FP, 0.f);
        for (int i = 0; i < n_mels; ++i) {
            const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
            for (int f = 0; f < F; ++f) {
                const double freq = (sr / 2.0) * f / (F - 1);
                const double lower = (freq - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
                const double upper = (mel_f[i + 2] - freq) / (mel_f[i + 2] - mel_f[i + 1]);
                const double v = std::max(0.0, std::min(lower, upper));
                wt[(size_t)i * FP + f] = (float)(v * enorm);
            }
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (a.mel_wt) hipFree(a.mel_wt);
        a.mel_wt = nullptr;
        HIPCHK(h, hipMalloc(&a.mel_wt, wt.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(a.mel_wt, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
        a.sr = sr; a.n_fft = n_fft; a.n_mels = n_mels; a.fmin = fmin; a.fmax = fmax;
    }
    WS(h, "an.lin_tf", float, (size_t)B * n_frames * FP, lin_tf);
    WS(h, "an.mel_tf", float, (size_t)B * n_frames * n_mels, mel_tf);
    HIPCHK(h, launch_mag_ft_to_tf(h->stream, lin, lin_tf, B, F, n_frames, FP));
    int rc = run_single(h, dense_group(lin_tf, FP, a.mel_wt, nullptr, mel_tf, n_mels, B * n_frames, n_mels, FP, ACT_NONE));
    if (rc) return rc;
    HIPCHK(h, launch_tf_to_ft(h->stream, mel_tf, mel, B, n_mels, n_frames, n_mels));
    return TTS_OK;
}

int tts_db_convert(tts_handle_t h, const float* in, size_t n, int mode, float ref_db, float max_db, float* out) {
    DeviceScope dev_scope(h);
    if (!h || !in || !out || mode < 0 || mode > 3) return fail(h, TTS_ERR_INVALID, "db_convert: bad arguments");
    if (n == 0) return TTS_OK;
    if (mode == 1) {
        // reference audio/conversion.py:47-49: AssertionError if any dB value < -100
        int* flag = nullptr;
        int rc = denorm_flag_arm(h, &flag);
        if (rc) return rc;
        HIPCHK(h, launch_any_below(h->stream, in, n, -100.0f, flag));
        if ((rc = denorm_flag_read(h))) return rc;
    }
    HIPCHK(h, launch_db_convert(h->stream, in, out, n, mode, ref_db, max_db));
    return TTS_OK;
}

// Host-only view of the Griffin-Lim work-item planner (no GPU needed): items[n][4] = {utterance, first frame, frames, slot word}
// in the order the workgroups draw them (at most max_items are written), *ring_frames = frames the kernel's LDS ring holds;
// returns the number of items or a negative status.  n_frames: the lengths of a ragged batch (T is then their maximum) or null.
static int debug_gl_plan(const int32_t* n_frames, int T, int B, int win_length, int hop_length, int n_workers, int* items, int max_items,
                         int* ring_frames) {
    for (int b = 0; n_frames && b < B; ++b) {
        if (n_frames[b] < 1) return TTS_ERR_INVALID;
        T = std::max(T, (int)n_frames[b]);
    }
    if (T < 1 || B < 1 || win_length < 2 || win_length > TTS_GL_NFFT || hop_length < 1 || n_workers < 1 || !items || max_items < 0)
        return TTS_ERR_INVALID;
    const int ring = gl_stream_ring_frames(win_length, hop_length);
    if ((win_length + hop_length - 1) / hop_length > 8 || ring < 1) return TTS_ERR_UNSUPPORTED;
    const int n_stage = gl_iters_per_launch(3, win_length, hop_length, 0, 0);   // the handle's default launch form (option "gl_pair")
    std::vector<GlItem> v;
    int slots = 0;
    const int n = gl_plan_items(n_frames, T, B, win_length, hop_length, n_workers, n_stage, 0, 0, &v, &slots);
    if (ring_frames) *ring_frames = ring;
    std::memcpy(items, v.data(), (size_t)std::min(n, max_items) * sizeof(GlItem));
    return n;
}

int tts_debug_gl_plan(int T, int B, int win_length, int hop_length, int n_workers, int* items, int max_items, int* ring_frames) {
    return debug_gl_plan(nullptr, T, B, win_length, hop_length, n_workers, items, max_items, ring_frames);
}

// The same for a ragged batch (tts_griffin_lim_ragged): n_frames[b] frames in utterance b.
int tts_debug_gl_plan_ragged(const int32_t* n_frames, int B, int win_length, int hop_length, int n_workers, int* items, int max_items,
                             int* ring_frames) {
    return n_frames ? debug_gl_plan(n_frames, 0, B, win_length, hop_length, n_workers, items, max_items, ring_frames) : TTS_ERR_INVALID;
}

}  // extern "C"
