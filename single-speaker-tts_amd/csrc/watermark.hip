// The audio watermark: a keyed spread-spectrum carrier under a block envelope, embedded into and searched for in batches of mono
// waveforms.  No reference counterpart.  include/sstts_hip.h has the definition in full and watermark_plan.h every formula; the
// embedder is individually rounded IEEE double operations and the detector integer sums, so both are the bits of
// tests/watermark_oracle.py.
//
// Embed, two streaming passes over a row (a third where records are asked for):
//   wm_blockmax_kernel   E of every block of 64 samples, one wave a block
//   wm_embed_kernel      e = min(E[k - 1], E[k], E[k + 1]), the carrier's sign, the marked sample; one partial a tile
//   wm_stats_kernel      a row's record out of its tiles' partials
// Detect, the correlation search over D offsets.  a_q(d) depends on d through d mod L (the phase) and a shift of whole chips, so the
// chip sums are made once a phase and cross-correlated with the sign sequence: N D / L multiply-adds a row instead of N D.
//   wm_signs_kernel      the chips' signs, one bit each, once a call (they depend on the key alone)
//   wm_blockmax_kernel   E as above
//   wm_v_kernel          v of every sample, int8
//   wm_chips_kernel      A_f[i] of every phase f, int16, and the sum of its squares a tile, int64
//   wm_corr_kernel       a workgroup per (row, phase, range of shifts): tiles of chip sums and packed signs in LDS, a thread per
//                        (shift, sub-range of the tile), an int32 partial per run of a symbol's chips inside a tile, int64 sums per
//                        (thread, bit) in LDS; then S[d][:] and T[d]
//   wm_pick_kernel       a workgroup a row: the lowest d with the largest T, its energy, payload and sums
// No atomics, nothing uploaded, no host wait; every loop bound is a host value that travelled in the launch.
#include "api_internal.h"
#include "watermark_plan.h"

// y = x + (G e) s is a product, an exact product and a sum (tests/watermark_oracle.py); the file is also built with -ffp-contract=off
#pragma clang fp contract(off)

namespace tts {

struct WmLens {
    int n[WM_UTTS];
};

// what the embedder knows of a tile of one row
struct WmPartial {
    int marked;
    float peak;
};

// E[b][k] for k < wm_blocks(n[b]).  A workgroup takes a tile of 64 blocks, a wave 16 of them.
__global__ __launch_bounds__(WM_THREADS) void wm_blockmax_kernel(const float* __restrict__ wav, size_t row, WmLens lens, float* __restrict__ E, size_t e_row) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = lens.n[b];
    const long long first = (long long)blockIdx.x * WM_TILE;
    if (first >= n) return;
    const float* x = wav + (size_t)b * row;
    float m[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const long long i = first + (long long)(wave * 16 + j) * WM_BLOCK + lane;
        m[j] = i < n ? wm_magnitude(x[i]) : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        float v = m[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
        const long long k = first / WM_BLOCK + wave * 16 + j;
        if (lane == 0 && k < wm_blocks(n)) E[(size_t)b * e_row + (size_t)k] = v;
    }
}

// the envelope of sample i of a row of n samples out of its E
__device__ __forceinline__ float wm_env_at(const float* __restrict__ E, long long i, long long n) {
    const long long k = i / WM_BLOCK, nb = wm_blocks(n);
    const float a = k >= 1 ? E[k - 1] : 0.0f, c = k + 1 < nb ? E[k + 1] : 0.0f;
    return wm_min3(a, E[k], c);
}

// APART: out is another buffer, and every element of its rows is written (what lies at or behind n[b] as a copy); in place only
// the marked samples are.
template <bool APART>
__global__ __launch_bounds__(WM_THREADS) void wm_embed_kernel(const float* wav, float* out /* may equal wav */, size_t row, int N, WmLens lens, WmParams w,
                                                              const float* __restrict__ E, size_t e_row, WmPartial* __restrict__ partial,
                                                              size_t partial_row) {
    __shared__ int s_marked[WM_THREADS / 64];
    __shared__ float s_peak[WM_THREADS / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    const long long n = lens.n[b];
    const long long first = (long long)blockIdx.x * WM_TILE;
    if (first >= (APART ? (long long)N : n)) return;   // (uniform)
    const float* x = wav + (size_t)b * row;
    float* y = out + (size_t)b * row;
    const float* Eb = E + (size_t)b * e_row;
    int marked = 0;
    float peak = 0.0f;
#pragma unroll 4
    for (int j = 0; j < WM_TILE / WM_THREADS; ++j) {
        const long long i = first + j * WM_THREADS + t;
        if (i < n) {
            const float xf = x[i];
            bool m;
            const float o = wm_mark(xf, wm_env_at(Eb, i, n), w.strength, wm_carrier_u32(w, (uint32_t)i), &m);
            if (APART || m) y[i] = o;
            marked += m;
            peak = fmaxf(peak, fabsf(o));   // (a NaN is passed over)
        } else if (APART && i < N) {
            y[i] = x[i];
        }
    }
    if (partial) {   // (uniform)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            marked += __shfl_xor(marked, d, 64);
            peak = fmaxf(peak, __shfl_xor(peak, d, 64));
        }
        if ((t & 63) == 0) s_marked[t >> 6] = marked, s_peak[t >> 6] = peak;
        __syncthreads();
        if (t == 0 && first < n) {
            for (int k = 1; k < WM_THREADS / 64; ++k) marked += s_marked[k], peak = fmaxf(peak, s_peak[k]);
            partial[(size_t)b * partial_row + blockIdx.x] = WmPartial{marked, peak};
        }
    }
}

// One wave per row: the record of a row out of its tiles' partials.
__global__ __launch_bounds__(64) void wm_stats_kernel(WmLens lens, const WmPartial* __restrict__ partial, size_t partial_row,
                                                      tts_watermark_embed_stats_t* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long n_tiles = wm_tiles((long long)lens.n[b]);
    int marked = 0;
    float peak = 0.0f;
    for (long long i = lane; i < n_tiles; i += 64) {
        const WmPartial p = partial[(size_t)b * partial_row + (size_t)i];
        marked += p.marked;
        peak = fmaxf(peak, p.peak);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        marked += __shfl_xor(marked, d, 64);
        peak = fmaxf(peak, __shfl_xor(peak, d, 64));
    }
    if (lane == 0) stats[b] = tts_watermark_embed_stats_t{lens.n[b], marked, peak, 0};
}

// v[b][i] for i < n[b]
__global__ __launch_bounds__(WM_THREADS) void wm_v_kernel(const float* __restrict__ wav, size_t row, WmLens lens, const float* __restrict__ E, size_t e_row,
                                                          int8_t* __restrict__ v) {
    const int b = blockIdx.y, t = threadIdx.x;
    const long long n = lens.n[b];
    const long long first = (long long)blockIdx.x * WM_TILE;
    if (first >= n) return;
    const float* x = wav + (size_t)b * row;
    const float* Eb = E + (size_t)b * e_row;
#pragma unroll 4
    for (int j = 0; j < WM_TILE / WM_THREADS; ++j) {
        const long long i = first + j * WM_THREADS + t;
        if (i < n) v[(size_t)b * row + (size_t)i] = (int8_t)wm_v(x[i], wm_env_at(Eb, i, n));
    }
}

// bit q of signs: 1 where c(q) = -1.  A wave makes 64 bits at once.
__global__ __launch_bounds__(WM_THREADS) void wm_signs_kernel(uint64_t key, long long words, uint32_t* __restrict__ signs) {
    const long long q = (long long)blockIdx.x * WM_THREADS + threadIdx.x;
    const unsigned long long mask = __ballot(wm_chip_negative(key, (uint64_t)q));
    if ((threadIdx.x & 63) == 0) {
        const long long wd = q >> 5;
        if (wd < words) signs[wd] = (uint32_t)mask;
        if (wd + 1 < words) signs[wd + 1] = (uint32_t)(mask >> 32);
    }
}

// A[b][f][i] for every i of the launched tiles (0 where no sample of the row falls into the chip) and the tile's sum of squares.
__global__ __launch_bounds__(WM_THREADS) void wm_chips_kernel(const int8_t* __restrict__ v, size_t row, WmLens lens, int L, int16_t* __restrict__ A,
                                                              size_t chips_pad, long long* __restrict__ epart, size_t e_tiles) {
    __shared__ long long s_sum[WM_THREADS / 64];
    const int b = blockIdx.z, f = blockIdx.y, t = threadIdx.x;
    const long long n = lens.n[b];
    const int8_t* vb = v + (size_t)b * row;
    int16_t* Ab = A + ((size_t)b * L + f) * chips_pad;
    long long sq = 0;
    for (int j = 0; j < WM_CORR_TILE / WM_THREADS; ++j) {
        const long long i = (long long)blockIdx.x * WM_CORR_TILE + j * WM_THREADS + t;
        const long long s0 = i * L - f;
        int a = 0;
        for (int u = 0; u < L; ++u) {
            const long long s = s0 + u;
            if (s >= 0 && s < n) {
                const int val = vb[s];
                a += u < L / 2 ? val : -val;
            }
        }
        Ab[i] = (int16_t)a;
        sq += (long long)(a * a);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d, 64);
    if ((t & 63) == 0) s_sum[t >> 6] = sq;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < WM_THREADS / 64; ++k) sq += s_sum[k];
        epart[((size_t)b * L + f) * e_tiles + blockIdx.x] = sq;
    }
}

// S[b][d][j] and T[b][d] for the offsets d = (range SW + shift) L + f of this workgroup.  SW: the shifts of a workgroup, a power of
// two; a thread takes shift t % SW and sub-range t / SW of every tile.
__global__ __launch_bounds__(WM_CORR_THREADS) void wm_corr_kernel(const int16_t* __restrict__ A, size_t chips_pad, const uint32_t* __restrict__ signs,
                                                                  long long sign_words, WmLens lens, int L, int C, int P, int D, int SW,
                                                                  long long* __restrict__ S, long long* __restrict__ T) {
    extern __shared__ long long wm_lds[];
    long long* slots = wm_lds;                                                            // [P][128]
    uint32_t* tile = reinterpret_cast<uint32_t*>(wm_lds + (size_t)P * WM_CORR_THREADS);   // WM_CORR_TILE int16
    uint32_t* sw = tile + WM_CORR_TILE / 2;                                               // the tile's sign words
    const int16_t* tile16 = reinterpret_cast<const int16_t*>(tile);
    const int b = blockIdx.z, f = blockIdx.y, t = threadIdx.x;
    const int NK = WM_CORR_THREADS / SW, sub = WM_CORR_TILE / NK;
    const int sl = t % SW, kk = t / SW;
    const long long w0 = (long long)blockIdx.x * SW, w = w0 + sl;
    const long long n_tiles = wm_corr_tiles((long long)lens.n[b], L);
    const uint32_t* Aw = reinterpret_cast<const uint32_t*>(A + ((size_t)b * L + f) * chips_pad);
    for (int j = 0; j < P; ++j) slots[j * WM_CORR_THREADS + t] = 0;
    constexpr int SIGN_WORDS = (WM_CORR_TILE + WM_CORR_THREADS) / 32 + 2;
    for (long long tl = 0; tl < n_tiles; ++tl) {
        const long long i0 = tl * WM_CORR_TILE;
        const long long wb = (i0 + w0) >> 5;
        __syncthreads();
        for (int k = t; k < WM_CORR_TILE / 2; k += WM_CORR_THREADS) tile[k] = Aw[i0 / 2 + k];
        if (t < SIGN_WORDS) sw[t] = wb + t < sign_words ? signs[wb + t] : 0u;
        __syncthreads();
        const long long q = i0 + (long long)kk * sub + w;
        int left = C - (int)(q % C);
        int j = (int)((q / C) % P);
        int bit = (int)(q - wb * 32);
        const int16_t* a = tile16 + kk * sub;
        int acc = 0;
        for (int x = 0; x < sub; ++x, ++bit) {
            const int av = a[x];
            acc += (sw[bit >> 5] >> (bit & 31)) & 1u ? -av : av;
            if (--left == 0) {
                slots[j * WM_CORR_THREADS + t] += acc;
                acc = 0;
                left = C;
                j = j + 1 == P ? 0 : j + 1;
            }
        }
        slots[j * WM_CORR_THREADS + t] += acc;
    }
    __syncthreads();
    // the sub-ranges' sums of a (shift, bit) into one; it stays in the first sub-range's slot for T
    for (int item = t; item < SW * P; item += WM_CORR_THREADS) {
        const int s2 = item % SW, j = item / SW;
        long long sum = 0;
        for (int k = 0; k < NK; ++k) sum += slots[j * WM_CORR_THREADS + k * SW + s2];
        slots[j * WM_CORR_THREADS + s2] = sum;
        const long long d = (w0 + s2) * L + f;
        if (d < D) S[((size_t)b * D + (size_t)d) * P + j] = sum;
    }
    __syncthreads();
    if (t < SW) {
        const long long d = w * L + f;
        if (d < D) {
            long long sum = 0;
            for (int j = 0; j < P; ++j) {
                const long long s = slots[j * WM_CORR_THREADS + t];
                sum += s < 0 ? -s : s;
            }
            T[(size_t)b * D + (size_t)d] = sum;
        }
    }
}

// A workgroup a row: the lowest d with the largest T, its record, and S[offset][:] where asked for.
__global__ __launch_bounds__(WM_THREADS) void wm_pick_kernel(WmLens lens, int L, int P, int D, const long long* __restrict__ S, const long long* __restrict__ T,
                                                             const long long* __restrict__ epart, size_t e_tiles, tts_watermark_detect_t* __restrict__ records,
                                                             long long* __restrict__ sums) {
    __shared__ long long s_val[WM_THREADS];
    __shared__ int s_d[WM_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    long long best = -1;
    int at = 0;
    for (int d = t; d < D; d += WM_THREADS) {
        const long long v = T[(size_t)b * D + d];
        if (v > best) best = v, at = d;
    }
    s_val[t] = best, s_d[t] = at;
    __syncthreads();
    for (int h = WM_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) {
            const long long v = s_val[t + h];
            const int d = s_d[t + h];
            if (v > s_val[t] || (v == s_val[t] && v >= 0 && d < s_d[t])) s_val[t] = v, s_d[t] = d;
        }
        __syncthreads();
    }
    const int offset = s_d[0];
    const long long score = s_val[0];
    __syncthreads();
    const long long n_tiles = wm_corr_tiles((long long)lens.n[b], L);
    long long e = 0;
    for (long long i = t; i < n_tiles; i += WM_THREADS) e += epart[((size_t)b * L + offset % L) * e_tiles + (size_t)i];
    s_val[t] = e;
    __syncthreads();
    for (int h = WM_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) s_val[t] += s_val[t + h];
        __syncthreads();
    }
    if (t < 64) {   // (P <= 32: the first wave)
        const long long s = t < P ? S[((size_t)b * D + offset) * P + t] : 0;
        if (sums && t < P) sums[(size_t)b * P + t] = s;
        const unsigned long long neg = __ballot(s < 0);
        if (t == 0) records[b] = tts_watermark_detect_t{offset, lens.n[b], score, s_val[0], (uint32_t)neg, 0u};
    }
}

}  // namespace tts

namespace tts_api {

static WmParams wm_params_of(const tts_watermark_t& p) {
    return WmParams{p.key, p.payload, p.payload_bits, p.chip, p.chips_per_symbol, p.strength};
}

// The workspaces of a tts_watermark_embed call on B rows of N samples; the partials only where records are asked for.
int watermark_scratch(tts_handle_t h, int B, int N, bool records, WmScratch* s) {
    WS(h, "wm.E", float, (size_t)B * (size_t)wm_blocks(N), E);
    *s = WmScratch{E, nullptr};
    if (records) {
        WS(h, "wm.partial", WmPartial, (size_t)B * (size_t)wm_tiles(N), partial);
        s->partial = partial;
    }
    return TTS_OK;
}

// On h->stream; everything has been checked (wm_embed_check).
int watermark_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_watermark_t& params,
                   tts_watermark_embed_stats_t* stats) {
    WmScratch s;
    const int rc = watermark_scratch(h, B, N, stats != nullptr, &s);
    if (rc) return rc;
    const WmParams w = wm_params_of(params);
    const size_t e_row = (size_t)wm_blocks(N), partial_row = (size_t)wm_tiles(N);
    const bool apart = out != wav;
    ProfScope ps(h, ST_WATERMARK, (int64_t)length_chunks(B, WM_UTTS) * (stats ? 3 : 2));
    for (int b0 = 0; b0 < B; b0 += WM_UTTS) {
        const int nb = std::min(WM_UTTS, B - b0);
        WmLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        const float* x = wav + (size_t)b0 * N;
        float* y = out + (size_t)b0 * N;
        float* E = s.E + (size_t)b0 * e_row;
        WmPartial* part = stats ? reinterpret_cast<WmPartial*>(s.partial) + (size_t)b0 * partial_row : nullptr;
        // (a launch needs a block: rows that hold nothing still get their records, and apart their copy)
        const dim3 grid((unsigned)std::max(1LL, wm_tiles(longest)), nb), all((unsigned)wm_tiles(N), nb);
        hipLaunchKernelGGL(wm_blockmax_kernel, grid, dim3(WM_THREADS), 0, h->stream, x, (size_t)N, lens, E, e_row);
        if (apart)
            hipLaunchKernelGGL(wm_embed_kernel<true>, all, dim3(WM_THREADS), 0, h->stream, x, y, (size_t)N, N, lens, w, E, e_row, part, partial_row);
        else
            hipLaunchKernelGGL(wm_embed_kernel<false>, grid, dim3(WM_THREADS), 0, h->stream, x, y, (size_t)N, N, lens, w, E, e_row, part, partial_row);
        if (stats) hipLaunchKernelGGL(wm_stats_kernel, dim3(nb), dim3(64), 0, h->stream, lens, part, partial_row, stats + b0);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

// On h->stream; everything has been checked (wm_detect_check).
static int watermark_detect_impl(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, const WmParams& w, int D,
                                 tts_watermark_detect_t* records, long long* scores, long long* sums) {
    const int L = w.chip, P = w.payload_bits, C = w.chips_per_symbol;
    const size_t e_row = (size_t)wm_blocks(N), chips_pad = (size_t)wm_chips_padded(N, L), e_tiles = (size_t)wm_corr_tiles(N, L);
    const long long sign_words = wm_sign_words(N, L, D);
    const int SW = wm_corr_shifts(D, L), ranges = wm_corr_ranges(D, L);
    WS(h, "wm.E", float, (size_t)B * e_row, E);
    WS(h, "wm.v", int8_t, (size_t)B * (size_t)N, v);
    WS(h, "wm.signs", uint32_t, (size_t)sign_words, signs);
    WS(h, "wm.chips", int16_t, (size_t)B * L * chips_pad, A);
    WS(h, "wm.energy", long long, (size_t)B * L * e_tiles, epart);
    WS(h, "wm.sums", long long, (size_t)B * D * P, S);
    long long* T = scores;
    if (!T) {
        WS(h, "wm.scores", long long, (size_t)B * D, Tws);
        T = Tws;
    }
    const size_t lds = wm_corr_lds(P);
    ProfScope ps(h, ST_WATERMARK, 1 + (int64_t)length_chunks(B, WM_UTTS) * 5);
    hipLaunchKernelGGL(wm_signs_kernel, dim3((unsigned)((sign_words * 32 + WM_THREADS - 1) / WM_THREADS)), dim3(WM_THREADS), 0, h->stream, w.key, sign_words, signs);
    for (int b0 = 0; b0 < B; b0 += WM_UTTS) {
        const int nb = std::min(WM_UTTS, B - b0);
        WmLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        const float* x = wav + (size_t)b0 * N;
        float* Eb = E + (size_t)b0 * e_row;
        int8_t* vb = v + (size_t)b0 * N;
        int16_t* Ab = A + (size_t)b0 * L * chips_pad;
        long long* eb = epart + (size_t)b0 * L * e_tiles;
        const dim3 grid((unsigned)std::max(1LL, wm_tiles(longest)), nb);
        hipLaunchKernelGGL(wm_blockmax_kernel, grid, dim3(WM_THREADS), 0, h->stream, x, (size_t)N, lens, Eb, e_row);
        hipLaunchKernelGGL(wm_v_kernel, grid, dim3(WM_THREADS), 0, h->stream, x, (size_t)N, lens, Eb, e_row, vb);
        hipLaunchKernelGGL(wm_chips_kernel, dim3((unsigned)wm_corr_tiles(longest, L), L, nb), dim3(WM_THREADS), 0, h->stream, vb, (size_t)N, lens, L, Ab, chips_pad,
                           eb, e_tiles);
        hipLaunchKernelGGL(wm_corr_kernel, dim3(ranges, L, nb), dim3(WM_CORR_THREADS), lds, h->stream, Ab, chips_pad, signs, sign_words, lens, L, C, P, D, SW,
                           S + (size_t)b0 * D * P, T + (size_t)b0 * D);
        hipLaunchKernelGGL(wm_pick_kernel, dim3(nb), dim3(WM_THREADS), 0, h->stream, lens, L, P, D, S + (size_t)b0 * D * P, T + (size_t)b0 * D, eb, e_tiles,
                           records + b0, sums ? sums + (size_t)b0 * P : nullptr);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_watermark_max_offsets(void) { return WM_MAX_OFFSETS; }

int tts_watermark_embed(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_watermark_t* params,
                        tts_watermark_embed_stats_t* stats) {
    DeviceScope dev_scope(h);
    WmParams p{};
    if (params) p = wm_params_of(*params);
    const std::string why = wm_embed_check(reinterpret_cast<uintptr_t>(wav), reinterpret_cast<uintptr_t>(out), B, N, n_samples, params ? &p : nullptr);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "watermark_embed: " + why);
    if (!h) return TTS_ERR_INVALID;
    return watermark_impl(h, wav, out, B, N, n_samples, *params, stats);
}

int tts_watermark_detect(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, const tts_watermark_t* params, int D,
                         tts_watermark_detect_t* records, int64_t* scores, int64_t* sums) {
    DeviceScope dev_scope(h);
    WmParams p{};
    if (params) p = wm_params_of(*params);
    const std::string why = wm_detect_check(reinterpret_cast<uintptr_t>(wav), reinterpret_cast<uintptr_t>(records), B, N, n_samples, params ? &p : nullptr, D,
                                            reinterpret_cast<uintptr_t>(scores), reinterpret_cast<uintptr_t>(sums));
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "watermark_detect: " + why);
    if (!h) return TTS_ERR_INVALID;
    return watermark_detect_impl(h, wav, B, N, n_samples, p, D, records, reinterpret_cast<long long*>(scores), reinterpret_cast<long long*>(sums));
}

int tts_set_watermark(tts_handle_t h, int enabled, const tts_watermark_t* params) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled) {
        const std::string why = params ? wm_params_check(wm_params_of(*params)) : std::string("a NULL pointer (params is required)");
        if (!why.empty()) return fail(h, TTS_ERR_INVALID, "set_watermark: " + why);
        h->settings.wm.params = *params;
    }
    h->settings.wm.enabled = enabled != 0;
    return TTS_OK;
}

}  // extern "C"
