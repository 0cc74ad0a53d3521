// Planner of the streaming Griffin-Lim kernel (gl_stream_kernel, griffin_lim.hip): host arithmetic only, see gl_plan.h.
#include "gl_plan.h"
#include <algorithm>
#include <cmath>
#include <utility>

namespace tts {

GlStreamGeom gl_stream_geom(int win, int hop) {
    GlStreamGeom g;
    g.wpad = (NFFT - win) >> 1;
    g.halo = (win + hop - 1) / hop - 1;
    // A frame's forward FFT runs `lag` indices behind its overlap-add: halo, or one more when the reflect padding of the
    // signal's first frame reaches exactly as far as halo frames make final (windows with ncol * hop == win)
    g.lag = (g.halo + 1) * hop > 2 * (MH - g.wpad) ? g.halo : g.halo + 1;
    const int c_lo = g.wpad >> 7, c_hi = (g.wpad + win - 1) >> 7;   // first / last 128-sample slot the window touches
    g.S = 128 * (c_hi - c_lo + 1);
    g.acc_len = g.S - hop;
    return g;
}

// a workgroup's LDS in front of its rings: the waves' exchange buffers (complex float) and the control words
static constexpr size_t GL_LDS_FIXED = (size_t)GL_NW * EX_CPLX * 2 * sizeof(float) + CT_SWORDS * sizeof(int);

// Frames the ring holds (0: the window / hop pair does not fit).  Lower bound: what keeps an index from overwriting ring
// positions that a slower wave may still read (see gl_stream_kernel), and the reflect-padded frames' reach; upper
// bound: LDS.  More frames only make the lap-end read path rarer.
int gl_stream_ring_frames(int win, int hop, int n_stage) {
    const GlStreamGeom g = gl_stream_geom(win, hop);
    if (g.acc_len < 0) return 0;   // hop > span: frames do not even touch (ncol = 1 with a hop beyond the padded slots)
    // (n_stage rings share what the exchange buffers leave of the budget)
    const int budget = (GL_LDS_BUDGET - (int)GL_LDS_FIXED) / (int)sizeof(float) / n_stage - g.acc_len - 132;
    int need = 9 + g.lag + (g.S + hop - 1) / hop + 1;
    const int reach = (g.S + win + 2 * hop + hop - 1) / hop;   // what a reflect-padded frame reads is still in the ring, within one lap
    need = std::max(need, std::max(reach, GL_NW));
    const int R = std::min(budget / hop, std::max(64, need));
    return R >= need ? R : 0;
}

size_t gl_stream_lds_bytes(int win, int hop, int ring_frames, int n_stage) {
    const GlStreamGeom g = gl_stream_geom(win, hop);
    return GL_LDS_FIXED + (size_t)(n_stage < 1 ? 1 : n_stage) * (size_t)((hop * ring_frames + g.acc_len + 128 + 3) & ~3) * sizeof(float);
}

void gl_build_wlane(const float* window, const float* rwss, int win, int hop, int T, float* out) {
    const GlStreamGeom g = gl_stream_geom(win, hop);
    const int t_ref = g.halo < T ? g.halo : T - 1;   // an interior frame (all `halo` neighbours either side exist) if there is one
    for (int c = 0; c < 16; ++c)
        for (int e = 0; e < 2; ++e)
            for (int lane = 0; lane < 64; ++lane) {
                const int nw = 2 * (lane + 64 * c) + e - g.wpad;
                const bool in = nw >= 0 && nw < win;
                const float w = in ? window[nw] * (0.5f / (float)MH) : 0.f;
                const float rw = in ? rwss[(size_t)t_ref * hop + g.wpad + nw] : 0.f;
                out[(0 * 64 + lane) * 32 + 2 * c + e] = w;
                out[(1 * 64 + lane) * 32 + 2 * c + e] = w * rw;
            }
}

// Work items of the streaming form.  The frames of all utterances, one after another, are dealt to the workgroups in
// contiguous pieces of equal COST; a piece that crosses the end of an utterance is two runs (the tail of one utterance
// and the head of the next).  What a run costs beyond its frames was measured per workgroup (round 6,
// profiles/r06_experiment_gl_cut.txt): at three iterations per launch every stage starts halo + lag indices before the
// next one's first frame -- 24 indices per run that carry 72 of a frame's 6 transforms, 12 frames' worth with start and
// drain, a little less at an utterance's end where the frames outside are skipped but the reflect-padded ones take the
// index-mapped path.  Until round 6 every utterance was cut alike into runs of one length (a multiple of the eight waves)
// and a rest: at T = 1000, B = 64 on 224 workgroups three runs of 296 frames and one of 112, so that 192 workgroups took
// one long run (640 us) and 32 two short ones (515 us) -- 4.7 % of the chip idle in every launch; on 256 workgroups three of
// 256 and one of 232 (572 / 515 us, 4.5 %).  The waveform's bits do not depend on the cut (every sample is summed over the
// frames that cover it in ascending order whatever run they are in: tests/test_gpu_audio.py).
namespace {
struct GlRun { int b, t0, len, ord = 0; };   // ord: the run's ordinal inside its utterance (by first frame), set once the cut stands
struct GlCutCost { double interior, edge; };   // per END of a run, in frames
GlCutCost gl_cut_cost(int halo, int lag, int n_stage) {
    // interior end: (halo + lag) / 2 * n_stage^2 transforms of the 2 n_stage a frame takes = (halo + lag) n_stage / 4
    // frames (6 at 4 / 4 / 3), measured 5.5 with the start and drain of the stream; an utterance's end: about half
    const double c = (halo + lag) * n_stage / 4.0;
    return GlCutCost{c * (5.5 / 6.0), c * 0.5};
}
// deals the frames to `W` workers with at most `M` cost each; returns false if they do not fit.  workers[w] = its runs
// lens: frames per utterance (null: T for all); no run is shorter than min(min_len, its utterance)
// STORE = false: the same walk without keeping the runs -- feasibility and makespan alone, no allocation.  The scan of the
// bound below prices its ~400 candidates this way -- and leaves one as soon as a worker's load reaches `give_up`, the best
// makespan so far, which it then cannot beat -- and deals only the winner (a call that stops at the end of the speech
// plans on the host while the stream that bounds the step waits: tts_synthesize, synth_main).
template <bool STORE>
bool gl_deal(const int* lens, int T, int B, int W, double M, const GlCutCost& cc, int min_len_all, std::vector<std::vector<GlRun>>& workers, double* makespan,
             double give_up = 1e300) {
    if (STORE) workers.assign((size_t)W, {});
    bool w_empty = true;   // (workers[w].empty() of the storing form)
    int b = 0, t = 0, w = 0;
    double load = 0.0, worst = 0.0;
    while (b < B) {
        if (w >= W) return false;
        const int Tb = lens ? lens[b] : T;
        const int min_len = std::min(Tb, min_len_all);
        const int rest = Tb - t;
        const double left = t > 0 ? cc.interior : cc.edge;
        const double whole = rest + left + cc.edge;                    // the rest of the utterance as one run
        if (load + whole <= M + 1e-9) {
            if (STORE) workers[w].push_back(GlRun{b, t, rest});
            w_empty = false;
            load += whole;
            ++b; t = 0;
            continue;
        }
        int len = (int)std::floor(M - load - left - cc.interior + 1e-9);   // a run that ends inside the utterance
        if (rest - len < min_len) len = rest - min_len;                     // (never leave a sliver to the next worker)
        if (len >= min_len) {
            if (STORE) workers[w].push_back(GlRun{b, t, len});
            load += len + left + cc.interior;
            t += len;
        } else if (w_empty) {
            return false;                                                   // M is smaller than the smallest run
        }
        worst = std::max(worst, load);
        if (!STORE && worst >= give_up) return false;
        ++w; load = 0.0; w_empty = true;
    }
    worst = std::max(worst, load);
    if (makespan) *makespan = worst;
    return true;
}
}  // namespace

// lens == null: T frames in every utterance, and every line below does what it did for one length
int gl_plan_items(const int* lens, int T, int B, int win, int hop, int n_workers, int n_stage, int force_runs, int force_run_len,
                  std::vector<GlItem>* items, int* slots_per_utt, int* workers_out) {
    auto len_of = [&](int b) { return lens ? lens[b] : T; };
    long long total_frames = 0;
    int T_min = len_of(0), T_top = len_of(0);
    for (int b = 0; b < B; ++b) {
        total_frames += len_of(b);
        T_min = std::min(T_min, len_of(b));
        T_top = std::max(T_top, len_of(b));
    }
    if (lens && T_min == T_top) {   // one length after all: the uniform cut, item for item
        lens = nullptr;
        T = T_top;
    }
    const GlStreamGeom g = gl_stream_geom(win, hop);
    n_stage = n_stage < 1 ? 1 : (n_stage > 3 ? 3 : n_stage);
    n_workers = n_workers < 1 ? 1 : n_workers;
    std::vector<std::vector<GlRun>> workers;
    // tests / experiments only (per-handle options "gl_runs" / "gl_run_len" behind "debug_hooks", api_handle.hip): every
    // utterance cut alike into runs of one length and a rest, one run per list entry
    int forced_len = 0;
    if (force_runs >= 1 && force_runs <= T_top) forced_len = ((T_top + force_runs - 1) / force_runs + GL_NW - 1) / GL_NW * GL_NW;
    if (force_run_len >= GL_NW) forced_len = force_run_len / GL_NW * GL_NW;
    if (forced_len > 0) {
        for (int t0 = 0; t0 < T_top; t0 += forced_len)
            for (int b = 0; b < B; ++b)
                if (t0 < len_of(b)) workers.push_back({GlRun{b, t0, std::min(forced_len, len_of(b) - t0)}});
    } else {
        const GlCutCost cc = gl_cut_cost(g.halo, g.lag, n_stage);
        // the shortest run: a round of the eight waves -- down to half a round where the workgroups outnumber the rounds (one
        // utterance on a whole chip: 250 runs of 4 frames instead of 125 of 8, Griffin-Lim 1.06 -> 0.92 ms per call at B = 1)
        const long long per_worker = total_frames / n_workers;
        const int min_len_all = (int)std::max<long long>(GL_NW / 2, std::min<long long>(GL_NW, per_worker));
        const int min_len = std::min(T_min, min_len_all);
        // the smallest makespan over a scan of the bound (the deal is greedy: a lower bound does not always give a lower result)
        const double total = (double)total_frames + (double)B * 2 * cc.edge;
        double lo = std::max(total / n_workers, (double)min_len + 2 * cc.edge), best_t = 1e300;
        std::vector<std::vector<GlRun>> none;
        int best_step = -1;
        double best_M = 0.0;
        for (int step = 0; step < 400; ++step) {
            const double M = lo * (1.0 + 0.0025 * step);
            double t = 0.0;
            if (!gl_deal<false>(lens, T, B, n_workers, M, cc, min_len_all, none, &t, best_t - 1e-9)) continue;
            if (t < best_t - 1e-9) { best_t = t; best_M = M; best_step = step; }
        }
        // a ragged batch: the bounds between the best step and the one before it, sixteen times as fine (utterance ends fall
        // anywhere in a share, so a step of the scan -- a quarter per cent, 6 frames of a share of 2600 -- is worth looking into)
        if (lens && best_step > 0) {
            for (int sub = 1; sub < 16; ++sub) {
                const double M = lo * (1.0 + 0.0025 * (best_step - 1 + sub / 16.0));
                double t = 0.0;
                if (!gl_deal<false>(lens, T, B, n_workers, M, cc, min_len_all, none, &t, best_t - 1e-9)) continue;
                if (t < best_t - 1e-9) { best_t = t; best_M = M; }
            }
        }
        if (best_step >= 0) gl_deal<true>(lens, T, B, n_workers, best_M, cc, min_len_all, workers, nullptr);   // the winner's runs
        if (workers.empty()) {   // (cannot happen: at twice the average every deal fits) one run per utterance
            for (int b = 0; b < B; ++b) workers.push_back({GlRun{b, 0, len_of(b)}});
        }
    }
    std::vector<int> runs_of((size_t)B, 0);
    // (every path above makes an utterance's runs in ascending order of their first frame: the ordinal is a count)
    for (auto& w : workers) for (GlRun& r : w) r.ord = runs_of[r.b]++;
    int spu = 1;
    for (int b = 0; b < B; ++b) spu = std::max(spu, runs_of[b]);
    auto item_of = [&](const GlRun& r) {   // slot of a run = its ordinal inside the utterance (by first frame)
        const int ord = r.ord;
        const int pad = ord == runs_of[r.b] - 1 ? spu - runs_of[r.b] : 0;
        return GlItem{r.b, r.t0, r.len, ord | (pad << 16)};
    };
    // table order = the order the persistent workgroups draw in: every worker's first run, then the runs that follow in
    // the order their workers come free (the shortest first runs first)
    typedef std::pair<double, const GlRun*> Start;
    const auto earlier = [](const Start& a, const Start& b) { return a.first < b.first; };
    items->clear();
    size_t depth = 0;
    for (const auto& w : workers) depth = std::max(depth, w.size());
    if (lens) {
        // a ragged batch: the workers' runs differ too much in length for "level by level" to be the order they come free in (one
        // worker is through three short utterances before another has finished its first long one, and would take that one's
        // second run).  Behind the first runs the table is in the order of the PLANNED start of every run, frames and per-run
        // cost counted: a worker that comes free finds the run planned for that moment -- its own, if the plan holds.
        std::vector<Start> rest;
        for (const auto& w : workers) {
            double before = 0.0;
            for (size_t d = 0; d < w.size(); ++d) {
                if (d == 0) items->push_back(item_of(w[d]));
                else rest.push_back({before, &w[d]});
                before += w[d].len + 11.0;
            }
        }
        std::stable_sort(rest.begin(), rest.end(), earlier);
        for (const auto& e : rest) items->push_back(item_of(*e.second));
        depth = 0;
    }
    for (size_t d = 0; d < depth; ++d) {
        std::vector<Start> level;
        for (const auto& w : workers) {
            if (w.size() <= d) continue;
            double before = 0.0;
            for (size_t q = 0; q < d; ++q) before += w[q].len;
            level.push_back({before, &w[d]});
        }
        std::stable_sort(level.begin(), level.end(), earlier);
        for (const auto& e : level) items->push_back(item_of(*e.second));
    }
    if (workers_out) {
        int nw = 0;
        for (const auto& w : workers) nw += !w.empty();
        *workers_out = nw;
    }
    if (slots_per_utt) *slots_per_utt = spu;
    return (int)items->size();
}

}  // namespace tts
