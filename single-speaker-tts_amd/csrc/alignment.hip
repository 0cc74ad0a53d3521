// Attention diagnostics: an alignment history [n_steps][B][Ts] reduced to one exact record per utterance (where the attention
// stood at every step, whether it reached the last token, jumped back, stalled, skipped, sat on padding, and how focused it
// was), and the sentence lengths of padded ids.  No reference counterpart.  include/sstts_hip.h has the definition in full and
// alignment_plan.h the cut; every statistic but one is an integer and that one is a sum in a fixed order, so the records are the
// bits of tests/alignment_oracle.py.
//
//   align_rows_kernel   one wave per row (s, b): every lane keeps the best candidate of the elements it loads -- in 16-byte loads
//                       wherever the row's address allows (align_cover) -- for the sentence [0, N) and for the padding [N, Ts)
//                       apart, as 64-bit keys whose maximum IS the argmax with numpy's rules (align_key: the first NaN, else the
//                       lowest index of the maximum); a wave maximum of each, and pos, peak (the element's own bits, loaded
//                       again) and off (the padding's key is the larger) are written per step
//   align_walk_kernel   one wave per utterance over pos[0 .. S) and peak: integer reductions for everything order-free, a wave
//                       prefix maximum of the run starts for the longest stall, the durations by integer atomics on the
//                       utterance's own row, and the focus sum as the one sequential walk (a lane-broadcast per step)
//   text_lengths_kernel one wave per row of ids
// The work is a few megabytes: two launches per 64 utterances, bound by launch latency and the walk, not by memory (DESIGN.md
// 4.14).  No floating-point atomics; no loop bound depends on data: the lengths travelled in the launch.
#include "api_internal.h"
#include "alignment_plan.h"

// the focus sum is a chain of double additions and nothing else; the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

static_assert(sizeof(tts_alignment_stats_t) == 56, "the record is twelve int32 and a double");

struct AlignLens {
    int n_sent[ALIGN_UTTS];
    int n_steps[ALIGN_UTTS];
};

__device__ __forceinline__ unsigned long long align_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int align_wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int align_wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int align_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sentence length of utterance b of the launch: the host's, or -- inside a synthesis call -- what tts_text_lengths left on
// the device, held to 1 .. Ts here because nothing on the host has seen it
__device__ __forceinline__ int align_n_sent(const AlignLens& lens, const int32_t* __restrict__ d_n_sent, int b0, int b, int Ts) {
    return d_n_sent ? min(max(d_n_sent[b0 + b], 1), Ts) : lens.n_sent[b];
}

// ali [..][B][Ts]; pos, peak, off [B][n_steps_max], never null (the caller's or the handle's).  Steps s < cover are visited;
// those at or behind n_steps[b] get pos -1 and peak 0 and read nothing.
__global__ __launch_bounds__(64 * ALIGN_ROWS) void align_rows_kernel(const float* __restrict__ ali, int B, int Ts, int b0, AlignLens lens,
                                                                    const int32_t* __restrict__ d_n_sent, int cover, int n_steps_max,
                                                                    int32_t* __restrict__ pos, float* __restrict__ peak,
                                                                    unsigned char* __restrict__ off) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int s = blockIdx.x * ALIGN_ROWS + (threadIdx.x >> 6);
    if (s >= cover) return;   // (no barrier below: a wave may leave)
    const size_t o = (size_t)(b0 + b) * n_steps_max + s;
    if (s >= lens.n_steps[b]) {
        if (lane == 0) {
            pos[o] = -1;
            peak[o] = 0.f;
            off[o] = 0;
        }
        return;
    }
    const int N = align_n_sent(lens, d_n_sent, b0, b, Ts);
    const float* row = ali + ((size_t)s * B + (size_t)(b0 + b)) * Ts;
    const AlignCover c = align_cover((int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3), Ts);
    unsigned long long text = 0, pad = 0;   // (no key is 0)
    auto take = [&](float v, int j) {
        const unsigned long long k = align_key(__float_as_uint(v), (uint32_t)j);
        if (j < N) text = k > text ? k : text;
        else pad = k > pad ? k : pad;
    };
    if (lane < c.head) take(row[lane], lane);
    const float4* vec = reinterpret_cast<const float4*>(row + c.head);
    for (int i = lane; i < c.vecs; i += 64) {
        const float4 v = vec[i];
        const int j = c.head + 4 * i;
        take(v.x, j);
        take(v.y, j + 1);
        take(v.z, j + 2);
        take(v.w, j + 3);
    }
    if (lane < c.tail) take(row[Ts - c.tail + lane], Ts - c.tail + lane);
    text = align_wave_max(text);
    pad = align_wave_max(pad);
    if (lane == 0) {
        const int p = align_key_index(text);   // (N >= 1: the sentence has a candidate)
        pos[o] = p;
        peak[o] = row[p];
        off[o] = pad > text ? 1 : 0;
    }
}

// One wave per utterance.  dur [B][Ts], never null.
__global__ __launch_bounds__(64) void align_walk_kernel(int Ts, int b0, AlignLens lens, const int32_t* __restrict__ d_n_sent, int n_steps_max,
                                                        const int32_t* __restrict__ pos, const float* __restrict__ peak,
                                                        const unsigned char* __restrict__ off, int32_t* __restrict__ dur,
                                                        tts_alignment_stats_t* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int S = lens.n_steps[b];
    const int N = align_n_sent(lens, d_n_sent, b0, b, Ts);
    const int32_t* p = pos + (size_t)(b0 + b) * n_steps_max;
    const float* pk = peak + (size_t)(b0 + b) * n_steps_max;
    const unsigned char* of = off + (size_t)(b0 + b) * n_steps_max;
    int32_t* d = dur + (size_t)(b0 + b) * Ts;
    for (int j = lane; j < Ts; j += 64) d[j] = 0;
    __threadfence();
    __syncthreads();
    // what needs no order: the first step on the last token, the furthest position, the steps on padding, the durations
    int end = INT32_MAX, reached = 0, off_text = 0;
    for (int s = lane; s < S; s += 64) {
        const int q = p[s];
        reached = max(reached, q);
        if (q == N - 1) end = min(end, s);
        off_text += of[s];
        if ((unsigned)q < (unsigned)N) atomicAdd(d + q, 1);
    }
    end = align_wave_min(end);
    reached = align_wave_max(reached);
    off_text = align_wave_sum(off_text);
    const int end_step = end == INT32_MAX ? -1 : end;
    const int E = end_step >= 0 ? end_step : S - 1;
    // the moves within the spoken part, the steps off the last token behind it, and the longest stall: a run starts at step 0
    // and wherever the position changes, and step s has stood s - (the last start at or before s) + 1 steps
    int backward = 0, max_back = 0, max_jump = 0, after_end = 0, stall = 0, carry = -1;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool in = s < S;
        const int q = in ? p[s] : 0;
        const int prev = (in && s > 0) ? p[s - 1] : q;
        const bool spoken = in && s <= E;
        if (spoken && s >= 1) {
            const int dd = q - prev;
            backward += dd < 0;
            max_back = max(max_back, -dd);
            max_jump = max(max_jump, dd);
        }
        if (in && end_step >= 0 && s > end_step && q != N - 1) ++after_end;
        int st = (spoken && (s == 0 || q != prev)) ? s : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(st, o, 64);
            if (lane >= o) st = max(st, t);
        }
        st = max(st, carry);
        if (spoken) stall = max(stall, s - st + 1);
        carry = __shfl(st, 63, 64);
    }
    backward = align_wave_sum(backward);
    max_back = align_wave_max(max_back);
    max_jump = align_wave_max(max_jump);
    after_end = align_wave_sum(after_end);
    stall = align_wave_max(stall);
    // the focus: ((peak[0] + peak[1]) + peak[2]) + ..., the one thing with an order -- every lane walks the same chain on values
    // broadcast from the lane that loaded them
    double focus = 0.0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const float mine = s0 + lane < S ? pk[s0 + lane] : 0.f;
        const int n = min(64, S - s0);   // (uniform)
#pragma unroll
        for (int l = 0; l < 64; ++l) {
            if (l < n) {
                const double v = (double)__uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(mine), l));
                focus = (s0 + l == 0) ? v : __dadd_rn(focus, v);
            }
        }
    }
    // the positions in front of the furthest one that no step stood on (the counters are complete: they are read past the
    // vector cache, behind the wave's own atomics)
    __threadfence();
    __syncthreads();
    int skipped = 0;
    for (int j = lane; j < reached; j += 64) skipped += __hip_atomic_load(d + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    skipped = align_wave_sum(skipped);
    if (lane == 0) {
        tts_alignment_stats_t r;
        r.n_sent = N;
        r.n_steps = S;
        r.reached = reached;
        r.end_step = end_step;
        r.backward = backward;
        r.max_back = max_back;
        r.max_jump = max_jump;
        r.longest_stall = stall;
        r.after_end = after_end;
        r.off_text = off_text;
        r.skipped = skipped;
        r.reserved = 0;
        r.focus_sum = focus;
        stats[b0 + b] = r;
    }
}

// n_sent[b] = 1 + the largest j with ids[b][j] != pad_id; 1 for a row of padding.  One wave per row.
__global__ __launch_bounds__(64 * ALIGN_ROWS) void text_lengths_kernel(const int32_t* __restrict__ ids, int B, int Ts, int pad_id,
                                                                      int32_t* __restrict__ n_sent) {
    const int b = blockIdx.x * ALIGN_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const int32_t* row = ids + (size_t)b * Ts;
    int last = 0;
    for (int j = lane; j < Ts; j += 64)
        if (row[j] != pad_id) last = j;   // (ascending per lane: the lane's largest)
    last = align_wave_max(last);
    if (lane == 0) n_sent[b] = last + 1;
}

}  // namespace tts

namespace tts_api {

// The scratch of a call on B utterances of n_steps_max steps and Ts positions: the stand-alone calls' set, or a synthesis call's.
int alignment_scratch(tts_handle_t h, bool in_call, int B, int n_steps_max, int Ts, AlignScratch* s) {
    WS(h, in_call ? "syn.ali_pos" : "ali.pos", int32_t, (size_t)B * n_steps_max, wpos);
    WS(h, in_call ? "syn.ali_peak" : "ali.peak", float, (size_t)B * n_steps_max, wpeak);
    WS(h, in_call ? "syn.ali_off" : "ali.off", unsigned char, (size_t)B * n_steps_max, woff);
    WS(h, in_call ? "syn.ali_dur" : "ali.dur", int32_t, (size_t)B * Ts, wdur);
    *s = AlignScratch{wpos, wpeak, woff, wdur};
    return TTS_OK;
}

// On h->stream; everything has been checked (alignment_check).  d_n_sent: the sentence lengths on the device (a synthesis call;
// n_sent is then not looked at, and the scratch is the synthesis calls' own) or null.
int alignment_impl(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                   const int32_t* d_n_sent, tts_alignment_stats_t* stats, int32_t* durations, int32_t* pos, float* peak) {
    AlignScratch s;
    const int rc = alignment_scratch(h, d_n_sent != nullptr, B, n_steps_max, Ts, &s);
    if (rc) return rc;
    int32_t* ppos = pos ? pos : s.pos;
    float* ppeak = peak ? peak : s.peak;
    int32_t* pdur = durations ? durations : s.dur;
    unsigned char* woff = s.off;
    ProfScope ps(h, ST_ALIGNMENT, align_launches(B));
    for (int b0 = 0; b0 < B; b0 += ALIGN_UTTS) {
        const int nb = std::min(ALIGN_UTTS, B - b0);
        AlignLens lens;
        fill_lengths(lens.n_sent, n_sent, b0, nb, Ts);
        const int longest = fill_lengths(lens.n_steps, n_steps, b0, nb, n_steps_max);
        // (the caller's pos and peak are written to their end: -1 and 0 behind an utterance's steps)
        const int cover = (pos || peak) ? n_steps_max : longest;
        hipLaunchKernelGGL(align_rows_kernel, dim3(align_row_blocks(cover), nb), dim3(64 * ALIGN_ROWS), 0, h->stream, alignments, B, Ts, b0,
                           lens, d_n_sent, cover, n_steps_max, ppos, ppeak, woff);
        hipLaunchKernelGGL(align_walk_kernel, dim3(nb), dim3(64), 0, h->stream, Ts, b0, lens, d_n_sent, n_steps_max, ppos, ppeak, woff, pdur,
                           stats);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

// The positions alone -- pos[s] for s < n_steps[b], what tts_token_times compares its path with -- in the scratch alignment_impl
// would use: one launch per 64 utterances, counted by the caller's profile scope.  run false: alignment_impl has just left them there.
int alignment_positions_impl(tts_handle_t h, bool in_call, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent,
                             const int32_t* n_steps, const int32_t* d_n_sent, bool run, const int32_t** pos) {
    AlignScratch s;
    const int rc = alignment_scratch(h, in_call, B, n_steps_max, Ts, &s);
    if (rc) return rc;
    *pos = s.pos;
    for (int b0 = 0; run && b0 < B; b0 += ALIGN_UTTS) {
        const int nb = std::min(ALIGN_UTTS, B - b0);
        AlignLens lens;
        fill_lengths(lens.n_sent, n_sent, b0, nb, Ts);
        const int longest = fill_lengths(lens.n_steps, n_steps, b0, nb, n_steps_max);
        hipLaunchKernelGGL(align_rows_kernel, dim3(align_row_blocks(longest), nb), dim3(64 * ALIGN_ROWS), 0, h->stream, alignments, B, Ts, b0,
                           lens, d_n_sent, longest, n_steps_max, s.pos, s.peak, s.off);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

int text_lengths_impl(tts_handle_t h, const int32_t* ids, int B, int Ts, int pad_id, int32_t* n_sent) {
    ProfScope ps(h, ST_ALIGNMENT, 1);
    hipLaunchKernelGGL(text_lengths_kernel, dim3((B + ALIGN_ROWS - 1) / ALIGN_ROWS), dim3(64 * ALIGN_ROWS), 0, h->stream, ids, B, Ts, pad_id,
                       n_sent);
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_alignment_stats(tts_handle_t h, const float* alignments, int n_steps_max, int B, int Ts, const int32_t* n_sent, const int32_t* n_steps,
                        tts_alignment_stats_t* stats, int32_t* durations, int32_t* pos, float* peak) {
    DeviceScope dev_scope(h);
    std::string why = alignment_check(alignments && stats, n_steps_max, B, Ts, n_sent, n_steps);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(stats) & 7) ||
                        ((reinterpret_cast<uintptr_t>(alignments) | reinterpret_cast<uintptr_t>(durations) | reinterpret_cast<uintptr_t>(pos) |
                          reinterpret_cast<uintptr_t>(peak)) & 3)))
        why = "stats must be 8-byte aligned, the other buffers 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "alignment_stats: " + why);
    if (!h) return TTS_ERR_INVALID;
    return alignment_impl(h, alignments, n_steps_max, B, Ts, n_sent, n_steps, nullptr, stats, durations, pos, peak);
}

int tts_text_lengths(tts_handle_t h, const int32_t* ids, int B, int Ts, int pad_id, int32_t* n_sent) {
    DeviceScope dev_scope(h);
    std::string why = text_lengths_check(ids && n_sent, B, Ts);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(n_sent)) & 3)) why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "text_lengths: " + why);
    if (!h) return TTS_ERR_INVALID;
    return text_lengths_impl(h, ids, B, Ts, pad_id, n_sent);
}

int tts_set_alignment_stats(tts_handle_t h, int enabled, int pad_id) {
    if (!h) return TTS_ERR_INVALID;
    h->settings.ali.enabled = enabled != 0;
    if (enabled) h->settings.ali.pad_id = pad_id;
    return TTS_OK;
}

int tts_synth_alignment_stats(tts_handle_t h, tts_alignment_stats_t* stats_host, int B) {
    DeviceScope dev_scope(h);
    if (!h || !stats_host) return TTS_ERR_INVALID;
    if (!h->ali.last_dev)
        return fail(h, TTS_ERR_INVALID, "synth_alignment_stats: the last tts_synthesize call was not made with tts_set_alignment_stats on");
    if (B != h->ali.last_B)
        return fail(h, TTS_ERR_INVALID, "synth_alignment_stats: the last call had " + std::to_string(h->ali.last_B) + " utterances");
    // Behind the call's decoder and statistics, on whichever stream they ran, and not behind its Griffin-Lim: the copy goes on a
    // non-blocking stream of its own (a copy on the null stream would wait for the handle's main stream, Griffin-Lim included).
    if (!h->ali.copy) HIPCHK(h, hipStreamCreateWithFlags(&h->ali.copy, hipStreamNonBlocking));
    HIPCHK(h, h->ali.done.wait(h->ali.copy));
    HIPCHK(h, hipMemcpyAsync(stats_host, h->ali.last_dev, (size_t)B * sizeof(tts_alignment_stats_t), hipMemcpyDeviceToHost, h->ali.copy));
    HIPCHK(h, hipStreamSynchronize(h->ali.copy));
    return TTS_OK;
}

}  // extern "C"
