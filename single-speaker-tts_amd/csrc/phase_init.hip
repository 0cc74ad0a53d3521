// Estimated initial phases for Griffin-Lim: a single pass that tracks spectral peaks from frame to frame (after Beauregard,
// Harish and Wyse's single-pass spectrogram inversion), handed to the Griffin-Lim launches as their `init_phase`.
// DESIGN.md 4.5.7 has the definition; tests/phase_oracle.py restates it sequentially and is the yardstick.
//   phases are turns in unsigned 32-bit fixed point, additions wrap, phi_{-1} = 0.  Per frame t, on the float32 magnitudes m:
//   peak j (m[j] > both neighbours):  phi_t[j] = phi_{t-1}[j] + adv,  adv = (uint32)floor(frac(hop (j + p) / n_fft) 2^32), p the
//                                     vertex of the parabola through the three values, in double, every operation on its own
//   bin k owned by peak j:            phi_t[k] = phi_t[j] + ((k - j) & 1) 2^31   (the walk right while m rises, else left, ends at j)
//   any other bin:                    phi_t[k] = phi_{t-1}[k]
//   u[k][t] = (float)(phi_t[k] >> 8) 2^-24
// Apart from adv everything is integer arithmetic, so the result has the same bits however the work is cut.  It is cut in time:
// with src = owner or self, phi_t[k] = phi_{t-1}[src_t(k)] + off_t(k), and such maps compose associatively.  Chunks of PE_CHUNK
// frames: (1) every chunk but an utterance's last composes its map from the identity, (2) one workgroup per utterance chains the
// chunk ends into the phases each chunk starts from, (3) every chunk runs its frames again from those and writes.  An utterance
// of one chunk takes step 3 alone.  Steps 1 and 3 are one kernel (pe_chunk_kernel) and one frame analysis (pe_frame).
// The walks are not loops: the bins where a walk to the right (left) stops are bit masks of 64 bins per word, a walk's end is
// the first set bit at or behind (the last at or in front of) the bin, found in the bin's own word or through a table of the
// next (previous) word that has a bit.  No loop bound and no wait depends on the magnitudes; NaN compares false, so a NaN bin is
// no peak and stops every walk.
// The frames are analysed in time-major rows (what the call pipeline holds, `magi`); the public (B, F, T) layout is transposed
// into such rows first, and the result -- time-major as well -- is transposed into the public (B, F, T) array.  Frames at or
// behind an utterance's end are neither read nor written by any of the kernels; the lengths travel by value, PE_UTTS utterances
// per launch.
#include "api_internal.h"
#include "phase_plan.h"

// adv is specified operation by operation in IEEE double: nothing here may be contracted (also built with -ffp-contract=off,
// build.py).
#pragma clang fp contract(off)

namespace tts {

constexpr int PE_THREADS = 256;
constexpr int PE_WAVES = PE_THREADS / 64;
constexpr int PE_FMAX = PE_MAX_NFFT / 2 + 1;                        // 2049 bins
constexpr int PE_PER = (PE_FMAX + PE_THREADS - 1) / PE_THREADS;     // bins a thread takes: k = i PE_THREADS + thread
constexpr int PE_WORDS = PE_PER * PE_WAVES;                         // 64-bin mask words, word = i PE_WAVES + wave
constexpr int PE_LDS_BINS = PE_PER * PE_THREADS;

struct PeLens {
    int n[PE_UTTS];   // frames of the utterance: the frames behind them are neither read nor written
};

// adv of a peak with the neighbours a, b, g at bin j.  (a fraction that is not finite -- a -Inf neighbour -- advances by 0,
// as in the oracle: the conversion is undefined there)
__device__ __forceinline__ unsigned pe_advance(float af, float bf, float gf, int j, double hop, double n_fft) {
    const double a = (double)af, b = (double)bf, g = (double)gf;
    const double p = 0.5 * (a - g) / ((a - 2.0 * b) + g);
    const double x = (hop * ((double)j + p)) / n_fft;
    const double fr = x - floor(x);
    if (!(fr >= 0.0 && fr < 1.0)) return 0u;
    return (unsigned)floor(fr * 4294967296.0);
}

struct PeShared {
    float m[PE_LDS_BINS + 1];              // the frame
    unsigned adv[PE_LDS_BINS];             // adv of the bins that are peaks
    unsigned long long stop_r[PE_WORDS];   // bit k: a walk to the right stops at k, !(m[k] < m[k+1])
    unsigned long long stop_l[PE_WORDS];   // bit k: a walk to the left stops at k, !(m[k] < m[k-1])
    unsigned long long peak[PE_WORDS];
    int next_r[PE_WORDS + 1];              // the first word at or behind w with a bit in stop_r
    int prev_l[PE_WORDS + 1];              // the last word at or in front of w with a bit in stop_l
    unsigned state_o[2][PE_LDS_BINS];      // the chunk's map so far, offsets (COMPOSE) or the phases (otherwise), double-buffered
    unsigned short state_s[2][PE_LDS_BINS];   // the chunk's map so far, source bins (COMPOSE)
};

// One frame, `row` in registers (bin i PE_THREADS + thread in row[i]; bins >= F hold anything): -> src[i], off[i] of the
// thread's bins.  Called by all threads of the workgroup; three barriers.
__device__ __forceinline__ void pe_frame(PeShared& sh, const float (&row)[PE_PER], int F, int nw, double hop, double n_fft, int (&src)[PE_PER],
                                         unsigned (&off)[PE_PER]) {
    const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) sh.m[i * PE_THREADS + tid] = row[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) {
        const int k = i * PE_THREADS + tid;
        const int w = i * PE_WAVES + wave;
        if (w < nw) {   // (wave-uniform)
            const bool in = k < F;
            const float b = in ? sh.m[k] : 0.f;
            const float a = (in && k > 0) ? sh.m[k - 1] : 0.f;
            const float g = (in && k < F - 1) ? sh.m[k + 1] : 0.f;
            const bool up = in && k < F - 1 && b < g;
            const bool down = in && k > 0 && b < a;
            const bool pk = in && k > 0 && k < F - 1 && b > a && b > g;
            if (pk) sh.adv[k] = pe_advance(a, b, g, k, hop, n_fft);
            const unsigned long long mr = __ballot(!up), ml = __ballot(!down), mp = __ballot(pk);
            if ((tid & 63) == 0) {
                sh.stop_r[w] = mr;
                sh.stop_l[w] = ml;
                sh.peak[w] = mp;
            }
        }
    }
    __syncthreads();
    if (tid < nw) {   // (nw <= 36 words: every one has a bit -- bins >= F stop both walks, bin F - 1 the right one, bin 0 the left)
        int nr = nw - 1, pl = 0;
        for (int w = nw - 1; w >= tid; --w)
            if (sh.stop_r[w] != 0ull) nr = w;
        for (int w = 0; w <= tid; ++w)
            if (sh.stop_l[w] != 0ull) pl = w;
        sh.next_r[tid] = nr;
        sh.prev_l[tid] = pl;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) {
        const int k = i * PE_THREADS + tid;
        int s = k;
        unsigned o = 0u;
        if (k < F) {
            const int w = k >> 6, bit = k & 63;
            if ((sh.peak[w] >> bit) & 1ull) {
                o = sh.adv[k];
            } else {
                // the end of the walk to the right: the first stop at or behind k (bin F - 1 always stops: w + 1 < nw below)
                unsigned long long mk = sh.stop_r[w] & (~0ull << bit);
                int we = w;
                if (mk == 0ull) {
                    we = sh.next_r[w + 1];
                    mk = sh.stop_r[we];
                }
                int e = we * 64 + (__ffsll((long long)mk) - 1);
                bool owned = e < F && ((sh.peak[e >> 6] >> (e & 63)) & 1ull);
                if (!owned) {
                    // ... to the left: the last stop at or in front of k (bin 0 always stops: w >= 1 below)
                    mk = sh.stop_l[w] & (~0ull >> (63 - bit));
                    we = w;
                    if (mk == 0ull) {
                        we = sh.prev_l[w - 1];
                        mk = sh.stop_l[we];
                    }
                    e = we * 64 + 63 - __clzll((long long)mk);
                    owned = (sh.peak[e >> 6] >> (e & 63)) & 1ull;
                }
                if (owned) {
                    s = e;
                    o = sh.adv[e] + (((unsigned)(k - e) & 1u) << 31);
                }
            }
        }
        src[i] = s;
        off[i] = o;
    }
}

// One chunk of PE_CHUNK frames of one utterance; grid (chunks, utterances).  spec [nb][T][stride], time-major rows.
//   COMPOSE: the chunk's map from the identity -> map_s / map_o [nb][n_chunks][F]; an utterance's last chunk has none.
//   otherwise: the frames again from start [nb][n_chunks][F] (chunk 0 and start == null: from 0) -> u [nb][T][u_stride], float.
template <bool COMPOSE>
__global__ __launch_bounds__(PE_THREADS) void pe_chunk_kernel(const float* __restrict__ spec, PeLens lens, int T, int F, int stride, int n_chunks,
                                                              double hop, double n_fft, unsigned short* __restrict__ map_s,
                                                              unsigned* __restrict__ map_o, const unsigned* __restrict__ start,
                                                              float* __restrict__ u, int u_stride) {
    __shared__ PeShared sh;
    const int tid = threadIdx.x;
    const int c = blockIdx.x, b = blockIdx.y;
    const int n = lens.n[b];
    const int t0 = c * PE_CHUNK;
    const int t1 = min(n, t0 + PE_CHUNK);
    if (COMPOSE ? (t0 + PE_CHUNK >= n) : (t0 >= n)) return;   // (uniform: the last chunk's map is nobody's start)
    const int nw = (F + 63) >> 6;
    const size_t at = ((size_t)b * n_chunks + c) * F;
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) {
        const int k = i * PE_THREADS + tid;
        if (COMPOSE) {
            sh.state_s[0][k] = (unsigned short)k;
            sh.state_o[0][k] = 0u;
        } else {
            sh.state_o[0][k] = (c > 0 && k < F) ? start[at + k] : 0u;
        }
    }
    const float* p = spec + ((size_t)b * T + t0) * stride;
    float* q = COMPOSE ? nullptr : u + ((size_t)b * T + t0) * u_stride;
    float row[PE_PER], nxt[PE_PER];
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) {
        const int k = i * PE_THREADS + tid;
        nxt[i] = k < F ? p[k] : 0.f;
    }
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int i = 0; i < PE_PER; ++i) row[i] = nxt[i];
        if (t + 1 < t1) {   // (the next frame is on its way while this one is analysed)
            p += stride;
#pragma unroll
            for (int i = 0; i < PE_PER; ++i) {
                const int k = i * PE_THREADS + tid;
                nxt[i] = k < F ? p[k] : 0.f;
            }
        }
        int src[PE_PER];
        unsigned off[PE_PER];
        pe_frame(sh, row, F, nw, hop, n_fft, src, off);   // (its first barrier also orders the state's writes before the reads below)
#pragma unroll
        for (int i = 0; i < PE_PER; ++i) {
            const int k = i * PE_THREADS + tid;
            if (k < F) {
                const unsigned v = sh.state_o[cur][src[i]] + off[i];
                sh.state_o[cur ^ 1][k] = v;
                if (COMPOSE) sh.state_s[cur ^ 1][k] = sh.state_s[cur][src[i]];
                else q[k] = (float)(v >> 8) * 0x1p-24f;
            }
        }
        if (!COMPOSE) q += u_stride;
        cur ^= 1;
    }
    if (COMPOSE) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PE_PER; ++i) {
            const int k = i * PE_THREADS + tid;
            if (k < F) {
                map_s[at + k] = sh.state_s[cur][k];
                map_o[at + k] = sh.state_o[cur][k];
            }
        }
    }
}

// The chunk ends of one utterance, one after the other: start[c] = start[c-1][map_s[c-1]] + map_o[c-1], start[0] = 0 (not stored).
__global__ __launch_bounds__(PE_THREADS) void pe_chain_kernel(PeLens lens, int F, int n_chunks, const unsigned short* __restrict__ map_s,
                                                              const unsigned* __restrict__ map_o, unsigned* __restrict__ start) {
    __shared__ unsigned phi[2][PE_LDS_BINS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int nc = (lens.n[b] + PE_CHUNK - 1) / PE_CHUNK;   // the utterance's chunks, <= n_chunks
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) phi[0][i * PE_THREADS + tid] = 0u;
    int cur = 0;
    for (int c = 1; c < nc; ++c) {
        const size_t from = ((size_t)b * n_chunks + (c - 1)) * F;
        int s[PE_PER];
        unsigned o[PE_PER];
#pragma unroll
        for (int i = 0; i < PE_PER; ++i) {
            const int k = i * PE_THREADS + tid;
            s[i] = k < F ? (int)map_s[from + k] : 0;
            o[i] = k < F ? map_o[from + k] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PE_PER; ++i) {
            const int k = i * PE_THREADS + tid;
            if (k < F) {
                const unsigned v = phi[cur][s[i]] + o[i];
                phi[cur ^ 1][k] = v;
                start[from + F + k] = v;
            }
        }
        cur ^= 1;
    }
}

// in [nb][R][in_stride] (its first C columns) -> out [nb][C][out_stride], out[b][c][r] = in[b][r][c], through a 32 x 33 tile.
// TIME_ROWS: the rows of `in` are frames, otherwise its columns are; frames at or behind lens.n[b] are neither read nor written.
template <bool TIME_ROWS>
__global__ __launch_bounds__(256) void pe_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, PeLens lens, int R, int C,
                                                           int in_stride, int out_stride) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int n = lens.n[b];
    const int r_end = TIME_ROWS ? n : R, c_end = TIME_ROWS ? C : n;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    if (r0 >= r_end || c0 >= c_end) return;   // (uniform)
    const float* p = in + (size_t)b * R * in_stride;
    float* q = out + (size_t)b * C * out_stride;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        if (r < r_end && c < c_end) tile[j][tx] = p[(size_t)r * in_stride + c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (r < r_end && c < c_end) q[(size_t)c * out_stride + r] = tile[tx][j];
    }
}

}  // namespace tts

namespace tts_api {

// The workspaces of an estimate of B utterances of T frames.  from_public: the input is (B, F, T) and is transposed first;
// gl_start: the estimate starts a Griffin-Lim call, which reads it from a workspace like a caller's init_phase (gl_init_phase).
int phase_estimate_scratch(tts_handle_t h, int B, int T, int n_fft, bool from_public, bool gl_start, PhaseScratch* s) {
    const int F = 1 + n_fft / 2, FP = gl_fp(n_fft);
    const int n_chunks = pe_chunks(T);
    *s = PhaseScratch{};
    WS(h, "pe.u_rows", float, (size_t)B * T * FP, u_rows);
    s->u_rows = u_rows;
    if (from_public) {
        WS(h, "pe.mag_rows", float, (size_t)B * T * FP, mag_rows);
        s->mag_rows = mag_rows;
    }
    if (n_chunks > 1) {
        WS(h, "pe.map_s", unsigned short, (size_t)B * n_chunks * F, ms);
        WS(h, "pe.map_o", unsigned, (size_t)B * n_chunks * F, mo);
        WS(h, "pe.start", unsigned, (size_t)B * n_chunks * F, st);
        s->map_s = ms; s->map_o = mo; s->start = st;
    }
    if (gl_start) {
        WS(h, "gl.init_est", float, (size_t)B * F * T, est);
        s->init_est = est;
    }
    return TTS_OK;
}

// Both layouts on h->stream: time_major = rows of `row_stride` floats ([B][T][row_stride]), otherwise the public (B, F, T).
// n_frames: HOST lengths or null (all T).  out: the public (B, F, T) array.  Everything has been checked (phase_check).
int phase_estimate_impl(tts_handle_t h, const float* mag, int B, int T, int row_stride, bool time_major, const int32_t* n_frames, int n_fft,
                        int hop, float* out) {
    const int F = 1 + n_fft / 2, FP = gl_fp(n_fft);
    const int n_chunks = pe_chunks(T);
    PhaseScratch s;
    const int rc = phase_estimate_scratch(h, B, T, n_fft, !time_major, false, &s);
    if (rc) return rc;
    ProfScope ps(h, ST_PHASE_INIT, (int64_t)length_chunks(B, PE_UTTS) * ((time_major ? 2 : 3) + (n_chunks > 1 ? 2 : 0)));
    const dim3 tile_grid_in((T + 31) / 32, (F + 31) / 32), tile_grid_out((F + 31) / 32, (T + 31) / 32);
    for (int b0 = 0; b0 < B; b0 += PE_UTTS) {
        const int nb = std::min(PE_UTTS, B - b0);
        PeLens lens;
        const int longest = fill_lengths(lens.n, n_frames, b0, nb, T);
        const float* rows = mag + (size_t)b0 * T * row_stride;
        int stride = row_stride;
        if (!time_major) {
            float* dst = s.mag_rows + (size_t)b0 * T * FP;
            hipLaunchKernelGGL(pe_transpose_kernel<false>, dim3(tile_grid_in.x, tile_grid_in.y, nb), dim3(256), 0, h->stream,
                               mag + (size_t)b0 * F * T, dst, lens, F, T, T, FP);
            rows = dst;
            stride = FP;
        }
        float* u = s.u_rows + (size_t)b0 * T * FP;
        const size_t at = (size_t)b0 * n_chunks * F;
        const int live_chunks = pe_chunks(longest);
        if (live_chunks > 1) {
            hipLaunchKernelGGL(pe_chunk_kernel<true>, dim3(live_chunks - 1, nb), dim3(PE_THREADS), 0, h->stream, rows, lens, T, F, stride, n_chunks,
                               (double)hop, (double)n_fft, s.map_s + at, s.map_o + at, (const unsigned*)nullptr, (float*)nullptr, 0);
            hipLaunchKernelGGL(pe_chain_kernel, dim3(nb), dim3(PE_THREADS), 0, h->stream, lens, F, n_chunks, s.map_s + at, s.map_o + at, s.start + at);
        }
        // (u's rows are FP floats apart whatever the input's stride)
        hipLaunchKernelGGL(pe_chunk_kernel<false>, dim3(live_chunks, nb), dim3(PE_THREADS), 0, h->stream, rows, lens, T, F, stride, n_chunks,
                           (double)hop, (double)n_fft, (unsigned short*)nullptr, (unsigned*)nullptr,
                           live_chunks > 1 ? (const unsigned*)(s.start + at) : (const unsigned*)nullptr, u, FP);
        hipLaunchKernelGGL(pe_transpose_kernel<true>, dim3(tile_grid_out.x, tile_grid_out.y, nb), dim3(256), 0, h->stream, u,
                           out + (size_t)b0 * F * T, lens, T, F, FP, T);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_phase_estimate(tts_handle_t h, const float* mag, int B, int T, const int32_t* n_frames, int n_fft, int hop_length, float* init_phase_out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const std::string why = phase_check(mag && init_phase_out, B, T, 1 + n_fft / 2, n_frames, n_fft, hop_length);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "phase_estimate: " + why);
    return phase_estimate_impl(h, mag, B, T, 0, false, n_frames, n_fft, hop_length, init_phase_out);
}

int tts_phase_estimate_rows(tts_handle_t h, const float* spec, int B, int T, int row_stride, const int32_t* n_frames, int n_fft, int hop_length,
                            float* init_phase_out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const std::string why = phase_check(spec && init_phase_out, B, T, row_stride, n_frames, n_fft, hop_length);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "phase_estimate_rows: " + why);
    return phase_estimate_impl(h, spec, B, T, row_stride, true, n_frames, n_fft, hop_length, init_phase_out);
}

int tts_phase_chunk_frames(void) { return PE_CHUNK; }

}  // extern "C"
