// Timing marks: an alignment history [n_steps][B][Ts] searched for its best monotone path -- a non-decreasing position per step
// that advances by at most J tokens a step -- and the path turned into the step every token starts at.  No reference
// counterpart.  include/sstts_hip.h has the definition in full and token_times_plan.h the cut; every quantity is an integer, so
// the results are the bits of tests/marks_oracle.py.
//
//   align_rows_kernel    (alignment.hip) the argmax positions, for `agree` alone
//   token_times_kernel   one workgroup per utterance.  Lane t holds columns t, t + 256, ...; row s of the table is made from row
//                        s - 1 in LDS (two rows of int64, J + 1 reads per cell), one barrier per row; a byte of direction
//                        per cell goes to LDS, or to the workspace
//                        "tt.dir" where the launch's longest utterance does not fit (tt_dir_in_lds).  The lowest maximum of the
//                        last row is a reduction over (value, column); lane 0 walks back S - 1 dependent reads; start, the
//                        counts and the record are again the whole workgroup's.
// Bound by latency, not by memory or arithmetic: S rows, each behind a barrier, its elements' load and its LDS reads, then S
// dependent reads of the walk back -- 0.56 us per step.  Requesting a row's elements one row ahead and reading four predecessors
// per LDS round trip were both measured and were no faster: neither is kept.  Integer arithmetic only; no atomics; no loop bound depends on device data: the lengths travelled in the launch.
#include "api_internal.h"
#include "token_times_plan.h"

namespace tts {

static_assert(sizeof(tts_token_times_stats_t) == 32, "the record is an int64 and six int32");

struct TtLens {
    int n_sent[TT_UTTS];
    int n_steps[TT_UTTS];
};

__device__ __forceinline__ int tt_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over the workgroup, in every lane; red: TT_THREADS / 64 ints of LDS, free again on return
__device__ __forceinline__ int tt_block_sum(int v, int* red) {
    v = tt_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TT_THREADS / 64; ++w) sum += red[w];
    __syncthreads();
    return sum;
}

// ali [..][B][Ts]; pos [B][n_steps_max] (align_rows_kernel); dir_ws: the directions of utterance b0 + b at dir_ws + (b0 + b) *
// dir_stride bytes (DIR_LDS: unused); d_n_sent: the sentence lengths on the device, or null; start [B][Ts + 1]; path
// [B][n_steps_max], never null (the caller's or the handle's).  Dynamic LDS: tt_lds_bytes(longest, Ts).
template <bool DIR_LDS>
__global__ __launch_bounds__(TT_THREADS) void token_times_kernel(const float* __restrict__ ali, int B, int Ts, int b0, TtLens lens,
                                                                 const int32_t* __restrict__ d_n_sent, int J, int n_steps_max,
                                                                 const int32_t* __restrict__ pos,
                                                                 unsigned char* __restrict__ dir_ws, size_t dir_stride,
                                                                 int32_t* __restrict__ start, int32_t* __restrict__ path,
                                                                 tts_token_times_stats_t* __restrict__ stats) {
    extern __shared__ __align__(8) unsigned char tt_lds[];
    __shared__ long long red_v[TT_THREADS / 64];
    __shared__ int red_j[TT_THREADS / 64];
    __shared__ int red[TT_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    // (the sentence length: the host's, or -- inside a synthesis call -- what tts_text_lengths left on the device, held to
    //  1 .. Ts here because nothing on the host has seen it; no loop is bounded by it: it masks the lane's TT_PASSES columns)
    const int S = lens.n_steps[b], N = d_n_sent ? min(max(d_n_sent[b0 + b], 1), Ts) : lens.n_sent[b];
    long long* rows = reinterpret_cast<long long*>(tt_lds);   // [2][Ts]
    unsigned char* dir = DIR_LDS ? tt_lds + tt_rows_bytes(Ts) : dir_ws + (size_t)(b0 + b) * dir_stride;   // [S][Ts]
    const uint32_t* col = reinterpret_cast<const uint32_t*>(ali) + (size_t)(b0 + b) * Ts;
    const size_t step = (size_t)B * Ts;

    uint32_t next[TT_PASSES];   // the elements of the row
    auto load = [&](int s) {
#pragma unroll
        for (int p = 0; p < TT_PASSES; ++p) {
            const int j = t + p * TT_THREADS;
            next[p] = j < N ? col[(size_t)s * step + j] : 0u;
        }
    };
    load(0);
#pragma unroll
    for (int p = 0; p < TT_PASSES; ++p) {
        const int j = t + p * TT_THREADS;
        if (j < N) rows[j] = j <= J ? (long long)tt_weight(next[p]) : -1ll;
    }
    for (int s = 1; s < S; ++s) {
        load(s);
        __syncthreads();   // row s - 1 is written, and row s - 2 -- this row's place -- is read
        const long long* prev = rows + (size_t)((s - 1) & 1) * Ts;
        long long* cur = rows + (size_t)(s & 1) * Ts;
        unsigned char* drow = dir + (size_t)s * Ts;
#pragma unroll
        for (int p = 0; p < TT_PASSES; ++p) {
            const int j = t + p * TT_THREADS;
            if (j < N) {
                long long best = -1;
                int bd = 0;
                const int dmax = min(J, j);
                for (int d = 0; d <= dmax; ++d) {   // ascending d and a strict comparison: the smallest d of the maximum
                    const long long v = prev[j - d];
                    if (v > best) {
                        best = v;
                        bd = d;
                    }
                }
                cur[j] = best < 0 ? -1ll : best + (long long)tt_weight(next[p]);
                drow[j] = (unsigned char)bd;
            }
        }
    }
    __syncthreads();

    // last: the lowest column of the maximum of the last row (column 0 is always reachable: the maximum is >= 0)
    const long long* fin = rows + (size_t)((S - 1) & 1) * Ts;
    long long bv = -2;
    int bj = 0;
#pragma unroll
    for (int p = 0; p < TT_PASSES; ++p) {   // ascending columns
        const int j = t + p * TT_THREADS;
        if (j < N && fin[j] > bv) {
            bv = fin[j];
            bj = j;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov > bv || (ov == bv && oj < bj)) {
            bv = ov;
            bj = oj;
        }
    }
    if ((t & 63) == 0) {
        red_v[t >> 6] = bv;
        red_j[t >> 6] = bj;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TT_THREADS / 64; ++w) {
        if (w == 0 || red_v[w] > bv || (red_v[w] == bv && red_j[w] < bj)) {
            bv = red_v[w];
            bj = red_j[w];
        }
    }
    const long long score = bv;
    const int last = bj;

    // the walk back: S - 1 dependent reads of one lane
    int32_t* q = path + (size_t)(b0 + b) * n_steps_max;
    if (t == 0) {
        int j = last;
        for (int s = S - 1; s >= 1; --s) {
            q[s] = j;
            j -= dir[(size_t)s * Ts + j];
        }
        q[0] = j;
    }
    for (int s = S + t; s < n_steps_max; s += TT_THREADS) q[s] = -1;
    __syncthreads();   // (a workgroup-wide fence: the path is in memory for every lane)

    // start[j] = the first step at or behind token j: step s is that for the tokens behind q[s-1] up to q[s] -- at most J + 1 of
    // them at step 0, at most J behind it -- and S for every token behind `last`
    int32_t* st = start + (size_t)(b0 + b) * (Ts + 1);
    const int32_t* ps = pos + (size_t)(b0 + b) * n_steps_max;
    int jumps = 0, moves = 0, agree = 0;
    for (int s = t; s < S; s += TT_THREADS) {
        const int here = q[s], before = s ? q[s - 1] : -1;
        for (int d = 0; d <= J; ++d)
            if (here - d > before) st[here - d] = s;
        if (s) {
            jumps += here - before > 1;
            moves += here > before;
        } else {
            jumps += here > 1;
        }
        agree += here == ps[s];
    }
    for (int j = last + 1 + t; j <= Ts; j += TT_THREADS) st[j] = S;
    jumps = tt_block_sum(jumps, red);
    moves = tt_block_sum(moves, red);
    agree = tt_block_sum(agree, red);
    if (t == 0) {
        tts_token_times_stats_t r;
        r.score = score;
        r.n_sent = N;
        r.n_steps = S;
        r.last = last;
        r.jumps = jumps;
        r.skipped = last - moves;   // the tokens 0 .. last that have a step are q[0] and one more per move
        r.agree = agree;
        stats[b0 + b] = r;
    }
}

}  // namespace tts

namespace tts_api {

// The scratch of a call on B utterances of n_steps_max steps and Ts positions: the stand-alone calls' set, or a synthesis call's
// (which also holds the results of a call whose caller gave no room for them).  dir: where no launch can keep its directions in LDS.
int token_times_scratch(tts_handle_t h, bool in_call, int B, int n_steps_max, int Ts, TokenTimesScratch* s) {
    WS(h, in_call ? "syn.tt_path" : "tt.path", int32_t, (size_t)B * n_steps_max, wpath);
    unsigned char* dir = nullptr;
    if (!tt_dir_in_lds(n_steps_max, Ts)) {   // (a chunk whose longest utterance is shorter may still fit: the launch decides)
        WS(h, in_call ? "syn.tt_dir" : "tt.dir", unsigned char, (size_t)B * tt_dir_bytes(n_steps_max, Ts), wdir);
        dir = wdir;
    }
    int32_t* start = nullptr;
    tts_token_times_stats_t* stats = nullptr;
    if (in_call) {
        WS(h, "syn.tt_start", int32_t, (size_t)B * (Ts + 1), wstart);
        WS(h, "syn.tt_stats", tts_token_times_stats_t, (size_t)B, wstats);
        start = wstart;
        stats = wstats;
    }
    *s = TokenTimesScratch{wpath, dir, start, stats};
    return TTS_OK;
}

// On h->stream; everything has been checked (token_times_check).  path: the caller's or null.  d_n_sent: the sentence lengths on
// the device (a synthesis call; n_sent is then not looked at, and the scratch is the synthesis calls' own) or null.  have_pos: the
// call's alignment statistics have left the positions in that scratch already.
int token_times_impl(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                     const int32_t* d_n_sent, bool have_pos, int max_jump, int32_t* start, int32_t* path, tts_token_times_stats_t* stats) {
    TokenTimesScratch sc;
    int rc = token_times_scratch(h, d_n_sent != nullptr, B, n_steps_max, Ts, &sc);
    if (rc) return rc;
    int32_t* q = path ? path : sc.path;
    const size_t dir_stride = tt_dir_bytes(n_steps_max, Ts);
    ProfScope ps(h, ST_ALIGNMENT, tt_launches(B) / (have_pos ? 2 : 1));
    const int32_t* pos = nullptr;
    if ((rc = alignment_positions_impl(h, d_n_sent != nullptr, alignments, n_steps_max, B, Ts, n_sent, n_steps, d_n_sent, !have_pos, &pos)))
        return rc;
    for (int b0 = 0; b0 < B; b0 += TT_UTTS) {
        const int nb = std::min(TT_UTTS, B - b0);
        TtLens lens;
        fill_lengths(lens.n_sent, n_sent, b0, nb, Ts);
        const int longest = fill_lengths(lens.n_steps, n_steps, b0, nb, n_steps_max);
        const size_t lds = tt_lds_bytes(longest, Ts);
        if (tt_dir_in_lds(longest, Ts))
            hipLaunchKernelGGL(token_times_kernel<true>, dim3(nb), dim3(TT_THREADS), lds, h->stream, alignments, B, Ts, b0, lens, d_n_sent,
                               max_jump, n_steps_max, pos, (unsigned char*)nullptr, (size_t)0, start, q, stats);
        else
            hipLaunchKernelGGL(token_times_kernel<false>, dim3(nb), dim3(TT_THREADS), lds, h->stream, alignments, B, Ts, b0, lens, d_n_sent,
                               max_jump, n_steps_max, pos, sc.dir, dir_stride, start, q, stats);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_token_times(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                    int max_jump, int32_t* start, int32_t* path, tts_token_times_stats_t* stats) {
    DeviceScope dev_scope(h);
    std::string why = token_times_check(alignments && start && stats, n_steps_max, B, Ts, n_sent, n_steps, max_jump);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(stats) & 7) ||
                        ((reinterpret_cast<uintptr_t>(alignments) | reinterpret_cast<uintptr_t>(start) | reinterpret_cast<uintptr_t>(path)) & 3)))
        why = "stats must be 8-byte aligned, the other buffers 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "token_times: " + why);
    why = token_times_unsupported(Ts);
    if (!why.empty()) return fail(h, TTS_ERR_UNSUPPORTED, "token_times: " + why);
    if (!h) return TTS_ERR_INVALID;
    return token_times_impl(h, alignments, n_steps_max, B, Ts, n_sent, n_steps, nullptr, false, max_jump, start, path, stats);
}

int tts_token_times_max_tokens(void) { return TT_MAX_TOKENS; }

int tts_set_token_times(tts_handle_t h, int enabled, int pad_id, int max_jump) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled && (max_jump < 1 || max_jump > TT_MAX_JUMP))
        return fail(h, TTS_ERR_INVALID, "set_token_times: max_jump = " + std::to_string(max_jump) + " is not in 1 .. " + std::to_string(TT_MAX_JUMP));
    h->settings.tt.enabled = enabled != 0;
    if (enabled) {
        h->settings.tt.pad_id = pad_id;
        h->settings.tt.max_jump = max_jump;
    }
    return TTS_OK;
}

int tts_synth_token_times(tts_handle_t h, int32_t* start_host, tts_token_times_stats_t* stats_host, int B) {
    DeviceScope dev_scope(h);
    if (!h || !start_host || !stats_host) return TTS_ERR_INVALID;
    if (!h->tt.last_start)
        return fail(h, TTS_ERR_INVALID, "synth_token_times: the last tts_synthesize call was not made with tts_set_token_times on");
    if (B != h->tt.last_B)
        return fail(h, TTS_ERR_INVALID, "synth_token_times: the last call had " + std::to_string(h->tt.last_B) + " utterances");
    // Behind the call's decoder and search, on whichever stream they ran, and not behind its Griffin-Lim: the copies go on the
    // non-blocking side stream the alignment statistics are fetched on.
    if (!h->ali.copy) HIPCHK(h, hipStreamCreateWithFlags(&h->ali.copy, hipStreamNonBlocking));
    HIPCHK(h, h->tt.done.wait(h->ali.copy));
    HIPCHK(h, hipMemcpyAsync(start_host, h->tt.last_start, (size_t)B * (size_t)(h->tt.last_Ts + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                             h->ali.copy));
    HIPCHK(h, hipMemcpyAsync(stats_host, h->tt.last_stats, (size_t)B * sizeof(tts_token_times_stats_t), hipMemcpyDeviceToHost, h->ali.copy));
    HIPCHK(h, hipStreamSynchronize(h->ali.copy));
    return TTS_OK;
}

}  // extern "C"
