// Short-time objective intelligibility: STOI (Taal et al. 2011) and ESTOI (Jensen and Taal 2016) of batches of time-aligned
// waveforms at 10 kHz (audio/metrics.py).  No reference counterpart.  include/sstts_hip.h has the definition in full: the frame
// energies, the kept frames and the compacted samples are individually rounded IEEE double operations, the bits of
// tests/stoi_oracle.py; the envelopes and the value are held to a bound.  Five launches per 64 rows, no host wait
// between them, no atomics; every loop bound is a host value that travelled in the launch or a count an earlier launch left
// in the row's record.
//
// stoi_energy_kernel: a workgroup owns STOI_ENERGY_FRAMES consecutive frames of one row and stages their samples in LDS as
//   floats, sample q at q + q / 128; lane f walks frame f, E = E + t * t with t = w[i] * x[i] in ascending i.
// stoi_scan_kernel: a workgroup per row.  The largest energy that is not NaN (a maximum: exact in any order), the threshold
//   Emax * 1e-4, then every lane counts the kept frames of its run of consecutive frames, an exclusive scan of the 256 counts
//   in LDS, and the lanes write their indices in ascending order.
// stoi_envelope_kernel: a workgroup owns STOI_GROUP kept frames of one row.  It rebuilds the windowed samples of the compacted
//   signals from the at most three source frames each needs; a frame of either signal is a real sequence of 512 points, taken as
//   256 complex ones, transformed in LDS (fft_lds_f64.h) and unfolded for the bins of the bands, which are summed in ascending
//   bin order.  Each signal has its own transform: what one holds cannot reach the other's envelopes (zeros stay zeros).
// stoi_segment_kernel: a workgroup owns STOI_SEG_CHUNK segments of one row, a lane a segment: both envelopes of the tile's frames
//   in LDS as [signal][band][frame], so the lanes' reads at one (band, t) are consecutive.  A lane leaves the sum of its
//   segment's terms in band order and the count of its degenerate terms.
// stoi_value_kernel: a wave per row adds the segment sums in segment order and writes the record.
#include "api_internal.h"
#include "fft_lds_f64.h"
#include "stoi_plan.h"

// E = E + t * t is a product and a sum (tests/stoi_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct StoiLens {
    int n[STOI_UTTS];
};
struct StoiWindow {
    double w[STOI_W];
};
struct StoiBands {
    int32_t e[STOI_J][2];
};

// ref points at the first row of the launch, E at its first row of `cap` energies
__global__ __launch_bounds__(STOI_ENERGY_FRAMES) void stoi_energy_kernel(const float* __restrict__ ref, size_t row, StoiLens lens, StoiWindow win,
                                                                         double* __restrict__ E, int cap) {
    extern __shared__ __align__(16) float stoi_sx[];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int frames = stoi_frames(lens.n[b]);
    const int m0 = blockIdx.x * STOI_ENERGY_FRAMES;
    if (m0 >= frames) return;   // (uniform)
    const int nf = min(STOI_ENERGY_FRAMES, frames - m0);
    const float* x = ref + (size_t)b * row + (size_t)m0 * STOI_H;
    const int count = (nf + 1) * STOI_H;            // the last sample of frame m0 + nf - 1 is sample count - 1 from x: inside the row
    for (int q = lane; q < count; q += STOI_ENERGY_FRAMES) stoi_sx[q + q / STOI_H] = x[q];
    __syncthreads();
    if (lane >= nf) return;
    const float* s = stoi_sx + lane * (STOI_H + 1);
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < STOI_W; ++i) {
        const double t = __dmul_rn(win.w[i], (double)s[i + i / STOI_H]);
        acc = __dadd_rn(acc, __dmul_rn(t, t));
    }
    E[(size_t)b * cap + m0 + lane] = acc;
}

// records, index and E point at the first row of the launch
__global__ __launch_bounds__(STOI_SCAN_LANES) void stoi_scan_kernel(StoiLens lens, const double* __restrict__ E, int cap,
                                                                    tts_stoi_record_t* __restrict__ records, int32_t* __restrict__ index) {
    __shared__ double s_max[STOI_SCAN_LANES];
    __shared__ int s_cnt[STOI_SCAN_LANES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int frames = stoi_frames(lens.n[b]);
    const double* e = E + (size_t)b * cap;
    int32_t* idx = index + (size_t)b * cap;
    double mx = 0.0;   // energies are sums of squares: never below 0
    for (int m = tid; m < frames; m += STOI_SCAN_LANES) {
        const double v = e[m];
        if (v > mx) mx = v;   // (false for a NaN)
    }
    s_max[tid] = mx;
    __syncthreads();
    for (int d = STOI_SCAN_LANES / 2; d >= 1; d >>= 1) {
        if (tid < d && s_max[tid + d] > s_max[tid]) s_max[tid] = s_max[tid + d];
        __syncthreads();
    }
    const double thr = __dmul_rn(s_max[0], 1e-4);
    const int run = stoi_scan_run(frames);
    const int first = min(frames, tid * run), last = min(frames, first + run);
    int cnt = 0;
    for (int m = first; m < last; ++m) cnt += e[m] > thr ? 1 : 0;
    s_cnt[tid] = cnt;
    __syncthreads();
    // inclusive scan of the lanes' counts (Hillis-Steele: 8 steps of 256 lanes)
    for (int d = 1; d < STOI_SCAN_LANES; d <<= 1) {
        const int add = tid >= d ? s_cnt[tid - d] : 0;
        __syncthreads();
        s_cnt[tid] += add;
        __syncthreads();
    }
    int at = s_cnt[tid] - cnt;
    for (int m = first; m < last; ++m)
        if (e[m] > thr) idx[at++] = m;
    if (tid == STOI_SCAN_LANES - 1) {
        const int kept = s_cnt[tid];
        records[b].frames = frames;
        records[b].kept = kept;
        records[b].segments = stoi_segments(kept);
    }
}

// The windowed sample i of kept frame m of a compacted signal: z = w[i] * xs[128 m + i], xs the sum in ascending k of the
// windowed samples of the at most two kept frames k that cover it.
__device__ __forceinline__ double stoi_z(const float* __restrict__ x, const int32_t* __restrict__ idx, const double* __restrict__ w, int kept, int m,
                                         int i) {
    double xs;
    if (i < STOI_H) {
        const double cur = __dmul_rn(w[i], (double)x[(size_t)idx[m] * STOI_H + i]);
        xs = m >= 1 ? __dadd_rn(__dmul_rn(w[i + STOI_H], (double)x[(size_t)idx[m - 1] * STOI_H + i + STOI_H]), cur) : cur;
    } else {
        const double cur = __dmul_rn(w[i], (double)x[(size_t)idx[m] * STOI_H + i]);
        xs = m + 1 < kept ? __dadd_rn(cur, __dmul_rn(w[i - STOI_H], (double)x[(size_t)idx[m + 1] * STOI_H + i - STOI_H])) : cur;
    }
    return __dmul_rn(w[i], xs);
}

// ref, deg, records, index and env point at the first row of the launch; env: [row][2][J][cap]
__global__ __launch_bounds__(STOI_ENV_LANES) void stoi_envelope_kernel(const float* __restrict__ ref, const float* __restrict__ deg, size_t row,
                                                                       StoiWindow win, StoiBands bands,
                                                                       const tts_stoi_record_t* __restrict__ records,
                                                                       const int32_t* __restrict__ index, int cap, double* __restrict__ env) {
    extern __shared__ __align__(16) double stoi_lds[];
    constexpr int HALF = STOI_NFFT / 2;   // the points of the complex transform that makes a real one of STOI_NFFT
    const int b = blockIdx.y, tid = threadIdx.x;
    const int kept = records[b].kept;
    const int m0 = blockIdx.x * STOI_GROUP;
    if (m0 >= kept) return;   // (uniform)
    const int g = min(STOI_GROUP, kept - m0);
    dcf* a = reinterpret_cast<dcf*>(stoi_lds);                       // [STOI_GROUP][2: ref, deg][HALF]
    dcf* tw = a + (size_t)STOI_GROUP * 2 * HALF;                    // [HALF]: exp(-2 pi i k / STOI_NFFT)
    double* w = reinterpret_cast<double*>(tw + HALF);               // [STOI_W]
    for (int k = tid; k < HALF; k += STOI_ENV_LANES) {
        double sn, cs;
        sincospi(-(double)k / (double)HALF, &sn, &cs);
        tw[k] = dcf{cs, sn};
    }
    for (int i = tid; i < STOI_W; i += STOI_ENV_LANES) w[i] = win.w[i];
    __syncthreads();
    const int32_t* idx = index + (size_t)b * cap;
    // a real frame z of STOI_NFFT points as the complex c[n] = z[2 n] + i z[2 n + 1], n < HALF: the second half of them is the padding
    for (int q = tid; q < g * 2 * (STOI_W / 2); q += STOI_ENV_LANES) {
        const int fs = q / (STOI_W / 2), n = q % (STOI_W / 2);
        const float* x = ((fs & 1) ? deg : ref) + (size_t)b * row;
        dcf* af = a + (size_t)fs * HALF;
        af[fft_f64_bitrev(n, 8)] = dcf{stoi_z(x, idx, w, kept, m0 + (fs >> 1), 2 * n), stoi_z(x, idx, w, kept, m0 + (fs >> 1), 2 * n + 1)};
        af[fft_f64_bitrev(n + STOI_W / 2, 8)] = dcf{0.0, 0.0};
    }
    fft_f64_lds<8, 2>(a, tw, g * 2);
    // C -> the spectrum of z: E[k] = (C[k] + conj C[HALF - k]) / 2, O[k] = (C[k] - conj C[HALF - k]) / (2 i), Z[k] = E[k] + tw[k] O[k]
    // (the bands lie in 1 <= k < HALF).  A signal of zeros gives zeros exactly: each signal has its own transform.
    for (int q = tid; q < g * 2 * STOI_J; q += STOI_ENV_LANES) {
        const int fs = q / STOI_J, j = q % STOI_J;
        const dcf* af = a + (size_t)fs * HALF;
        double sum = 0.0;
        for (int k = bands.e[j][0]; k < bands.e[j][1]; ++k) {
            const dcf p = af[k], n = af[HALF - k], t = tw[k];
            const double ere = 0.5 * (p.x + n.x), eim = 0.5 * (p.y - n.y);
            const double ore = 0.5 * (p.y + n.y), oim = 0.5 * (n.x - p.x);
            const double re = ere + (t.x * ore - t.y * oim), im = eim + (t.x * oim + t.y * ore);
            sum += re * re + im * im;
        }
        env[(((size_t)b * 2 + (fs & 1)) * STOI_J + j) * cap + m0 + (fs >> 1)] = sqrt(sum);
    }
}

// np.minimum: a NaN on either side is a NaN
__device__ __forceinline__ double stoi_min(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a < b ? a : b); }

// the term of one band of a STOI segment: x, y at [t], t < STOI_N; *degenerate counts a term that is 0 by rule
__device__ __forceinline__ double stoi_term(const double* __restrict__ x, const double* __restrict__ y, int* degenerate) {
    const double clip = 1.0 + 5.623413251903491;   // c = 1 + 10 ** (15 / 20)
    double sxx = 0.0, syy = 0.0;
    for (int t = 0; t < STOI_N; ++t) {
        sxx = __dadd_rn(sxx, __dmul_rn(x[t], x[t]));
        syy = __dadd_rn(syy, __dmul_rn(y[t], y[t]));
    }
    const double ny = sqrt(syy);
    if (ny == 0.0) {
        ++*degenerate;
        return 0.0;
    }
    const double a = __ddiv_rn(sqrt(sxx), ny);
    double sx = 0.0, sy = 0.0;
    for (int t = 0; t < STOI_N; ++t) {
        sx = __dadd_rn(sx, x[t]);
        sy = __dadd_rn(sy, stoi_min(__dmul_rn(a, y[t]), __dmul_rn(clip, x[t])));
    }
    const double mx = __ddiv_rn(sx, (double)STOI_N), my = __ddiv_rn(sy, (double)STOI_N);
    double cxy = 0.0, cxx = 0.0, cyy = 0.0;
    for (int t = 0; t < STOI_N; ++t) {
        const double dx = __dsub_rn(x[t], mx);
        const double dy = __dsub_rn(stoi_min(__dmul_rn(a, y[t]), __dmul_rn(clip, x[t])), my);
        cxy = __dadd_rn(cxy, __dmul_rn(dx, dy));
        cxx = __dadd_rn(cxx, __dmul_rn(dx, dx));
        cyy = __dadd_rn(cyy, __dmul_rn(dy, dy));
    }
    if (cxx == 0.0 || cyy == 0.0) {
        ++*degenerate;
        return 0.0;
    }
    return __ddiv_rn(cxy, __dmul_rn(sqrt(cxx), sqrt(cyy)));
}

// The rows of one signal's J x N block to mean 0 and norm 1: mean[j], norm[j] (0: the row becomes zeros).
__device__ __forceinline__ void stoi_row_stats(const double* __restrict__ v, int stride, double (&mean)[STOI_J], double (&norm)[STOI_J],
                                               int* degenerate) {
#pragma unroll
    for (int j = 0; j < STOI_J; ++j) {
        const double* r = v + (size_t)j * stride;
        double s = 0.0;
        for (int t = 0; t < STOI_N; ++t) s = __dadd_rn(s, r[t]);
        const double m = __ddiv_rn(s, (double)STOI_N);
        double c = 0.0;
        for (int t = 0; t < STOI_N; ++t) {
            const double d = __dsub_rn(r[t], m);
            c = __dadd_rn(c, __dmul_rn(d, d));
        }
        mean[j] = m;
        norm[j] = sqrt(c);
        if (c == 0.0) ++*degenerate;
    }
}

// column t of the row-normalised block, then to mean 0 and norm 1 itself (zeros where its centred norm is 0)
__device__ __forceinline__ void stoi_column(const double* __restrict__ v, int stride, int t, const double (&mean)[STOI_J],
                                            const double (&norm)[STOI_J], double (&col)[STOI_J], int* degenerate) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < STOI_J; ++j) {
        col[j] = norm[j] == 0.0 ? 0.0 : __ddiv_rn(__dsub_rn(v[(size_t)j * stride + t], mean[j]), norm[j]);
        s = __dadd_rn(s, col[j]);
    }
    const double m = __ddiv_rn(s, (double)STOI_J);
    double c = 0.0;
#pragma unroll
    for (int j = 0; j < STOI_J; ++j) {
        col[j] = __dsub_rn(col[j], m);
        c = __dadd_rn(c, __dmul_rn(col[j], col[j]));
    }
    const double n = sqrt(c);
    if (c == 0.0) ++*degenerate;
#pragma unroll
    for (int j = 0; j < STOI_J; ++j) col[j] = c == 0.0 ? 0.0 : __ddiv_rn(col[j], n);
}

// records, env, sums and degs point at the first row of the launch; sums / degs: [row][cap]
template <bool EXTENDED>
__global__ __launch_bounds__(STOI_SEG_CHUNK) void stoi_segment_kernel(const tts_stoi_record_t* __restrict__ records, const double* __restrict__ env,
                                                                      int cap, double* __restrict__ sums, int32_t* __restrict__ degs) {
    extern __shared__ __align__(16) double stoi_tile[];   // [2][STOI_J][TILE]
    constexpr int TILE = stoi_seg_tile_frames();
    const int b = blockIdx.y, lane = threadIdx.x;
    const int kept = records[b].kept, segments = stoi_segments(kept);
    const int s0 = blockIdx.x * STOI_SEG_CHUNK;
    if (s0 >= segments) return;   // (uniform)
    const int have = min(TILE, kept - s0);
    const double* e = env + (size_t)b * 2 * STOI_J * cap;
    for (int q = lane; q < 2 * STOI_J * have; q += STOI_SEG_CHUNK) {
        const int r = q / have, t = q % have;
        stoi_tile[r * TILE + t] = e[(size_t)r * cap + s0 + t];
    }
    __syncthreads();
    const int s = s0 + lane;
    if (s >= segments) return;
    const double* X = stoi_tile + lane;
    const double* Y = stoi_tile + STOI_J * TILE + lane;
    int degenerate = 0;
    double sum = 0.0;
    if (!EXTENDED) {
        for (int j = 0; j < STOI_J; ++j) sum = __dadd_rn(sum, stoi_term(X + j * TILE, Y + j * TILE, &degenerate));
    } else {
        double mx[STOI_J], nx[STOI_J], my[STOI_J], ny[STOI_J], cx[STOI_J], cy[STOI_J];
        stoi_row_stats(X, TILE, mx, nx, &degenerate);
        stoi_row_stats(Y, TILE, my, ny, &degenerate);
        for (int t = 0; t < STOI_N; ++t) {
            stoi_column(X, TILE, t, mx, nx, cx, &degenerate);
            stoi_column(Y, TILE, t, my, ny, cy, &degenerate);
#pragma unroll
            for (int j = 0; j < STOI_J; ++j) sum = __dadd_rn(sum, __dmul_rn(cx[j], cy[j]));
        }
        sum = __ddiv_rn(sum, (double)STOI_N);
    }
    sums[(size_t)b * cap + s] = sum;
    degs[(size_t)b * cap + s] = degenerate;
}

// records, sums and degs point at the first row of the launch
__global__ __launch_bounds__(64) void stoi_value_kernel(tts_stoi_record_t* __restrict__ records, const double* __restrict__ sums,
                                                        const int32_t* __restrict__ degs, int cap, int extended) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int segments = records[b].segments;
    const double* sm = sums + (size_t)b * cap;
    const int32_t* dg = degs + (size_t)b * cap;
    double total = 0.0;
    int degenerate = 0;
    for (int s0 = 0; s0 < segments; s0 += 64) {
        const int s = s0 + lane;
        const double v = s < segments ? sm[s] : 0.0;
        degenerate += s < segments ? dg[s] : 0;
        const int steps = min(64, segments - s0);   // (uniform)
        for (int l = 0; l < steps; ++l) total = __dadd_rn(total, __shfl(v, l, 64));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) degenerate += __shfl_xor(degenerate, off, 64);
    if (lane == 0) {
        records[b].degenerate = degenerate;
        records[b].value = segments == 0 ? __builtin_nan("") : __ddiv_rn(total, (double)(extended ? segments : STOI_J * segments));
    }
}

}  // namespace tts

namespace tts_api {

// The workspaces of a tts_stoi call on B rows of N samples; the kept frames and the envelopes only where the caller brings no
// room for them.
int stoi_scratch(tts_handle_t h, int B, int N, bool own_index, bool own_envelopes, StoiScratch* s) {
    const size_t cap = (size_t)std::max(1, stoi_frames(N));
    WS(h, "stoi.energy", double, (size_t)B * cap, energy);
    WS(h, "stoi.sums", double, (size_t)B * cap, sums);
    WS(h, "stoi.degs", int32_t, (size_t)B * cap, degs);
    *s = StoiScratch{energy, sums, degs, nullptr, nullptr};
    if (own_index) {
        WS(h, "stoi.index", int32_t, (size_t)B * cap, index);
        s->index = index;
    }
    if (own_envelopes) {
        WS(h, "stoi.env", double, (size_t)B * 2 * STOI_J * cap, env);
        s->env = env;
    }
    return TTS_OK;
}

// On h->stream; everything has been checked (stoi_check).
static int stoi_impl(tts_handle_t h, const float* ref, const float* deg, int B, int N, const int32_t* n_samples, int extended,
                     tts_stoi_record_t* records, int32_t* kept_index, double* envelopes) {
    StoiScratch s;
    const int rc = stoi_scratch(h, B, N, kept_index == nullptr, envelopes == nullptr, &s);
    if (rc) return rc;
    const int cap = stoi_frames(N);
    int32_t* index = kept_index ? kept_index : s.index;
    double* env = envelopes ? envelopes : s.env;
    StoiWindow win;
    stoi_window(win.w);
    StoiBands bands;
    stoi_bands(bands.e);
    ProfScope ps(h, ST_STOI, (int64_t)length_chunks(B, STOI_UTTS) * 5);
    for (int b0 = 0; b0 < B; b0 += STOI_UTTS) {
        const int nb = std::min(STOI_UTTS, B - b0);
        StoiLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        const int frames = stoi_frames(longest);   // the upper bound of every row's kept frames
        const float* pr = ref + (size_t)b0 * N;
        const float* pd = deg + (size_t)b0 * N;
        tts_stoi_record_t* rec = records + b0;
        double* E = s.energy + (size_t)b0 * cap;
        double* sm = s.sums + (size_t)b0 * cap;
        int32_t* dg = s.degs + (size_t)b0 * cap;
        int32_t* ix = index + (size_t)b0 * cap;
        double* ev = env + (size_t)b0 * 2 * STOI_J * cap;
        hipLaunchKernelGGL(stoi_energy_kernel, dim3(stoi_groups(frames, STOI_ENERGY_FRAMES), nb), dim3(STOI_ENERGY_FRAMES), stoi_energy_lds_bytes(),
                           h->stream, pr, (size_t)N, lens, win, E, cap);
        hipLaunchKernelGGL(stoi_scan_kernel, dim3(nb), dim3(STOI_SCAN_LANES), 0, h->stream, lens, E, cap, rec, ix);
        hipLaunchKernelGGL(stoi_envelope_kernel, dim3(stoi_groups(frames, STOI_GROUP), nb), dim3(STOI_ENV_LANES), stoi_env_lds_bytes(), h->stream, pr,
                           pd, (size_t)N, win, bands, rec, ix, cap, ev);
        const dim3 seg_grid(stoi_groups(stoi_segments(frames), STOI_SEG_CHUNK), nb);
        if (extended)
            hipLaunchKernelGGL(stoi_segment_kernel<true>, seg_grid, dim3(STOI_SEG_CHUNK), stoi_seg_lds_bytes(), h->stream, rec, ev, cap, sm, dg);
        else
            hipLaunchKernelGGL(stoi_segment_kernel<false>, seg_grid, dim3(STOI_SEG_CHUNK), stoi_seg_lds_bytes(), h->stream, rec, ev, cap, sm, dg);
        hipLaunchKernelGGL(stoi_value_kernel, dim3(nb), dim3(64), 0, h->stream, rec, sm, dg, cap, extended);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_stoi(tts_handle_t h, const float* ref, const float* deg, int B, int N, const int32_t* n_samples, int extended, tts_stoi_record_t* records,
             int32_t* kept_index, double* envelopes) {
    DeviceScope dev_scope(h);
    bool unsupported = false;
    const std::string why = stoi_check(reinterpret_cast<uintptr_t>(ref), reinterpret_cast<uintptr_t>(deg), reinterpret_cast<uintptr_t>(records),
                                       reinterpret_cast<uintptr_t>(kept_index), reinterpret_cast<uintptr_t>(envelopes), B, N, n_samples, extended,
                                       &unsupported);
    if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "stoi: " + why);
    if (!h) return TTS_ERR_INVALID;
    return stoi_impl(h, ref, deg, B, N, n_samples, extended, records, kept_index, envelopes);
}

int tts_stoi_frames(int n) { return stoi_frames(n); }

int tts_stoi_max_frames(void) { return STOI_MAX_FRAMES; }

int tts_stoi_window(double w[256]) {
    if (!w) return TTS_ERR_INVALID;
    stoi_window(w);
    return TTS_OK;
}

int tts_stoi_bands(int32_t edges[15][2]) {
    if (!edges) return TTS_ERR_INVALID;
    stoi_bands(edges);
    return TTS_OK;
}

}  // extern "C"
