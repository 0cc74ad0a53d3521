// The look-ahead peak limiter and the true-peak meter behind loudness (no reference counterpart).  include/sstts_hip.h has the
// definition in full and limiter_plan.h the taps, the gain rule and the tile arithmetic; every operation is an individually
// rounded IEEE double operation, so the results are the bits of tests/limiter_oracle.py.
//
//   lim_peak_kernel   a workgroup per tile of LIM_TILE samples: the samples and their 5 + 6 neighbours as doubles in LDS, the
//                     envelope per sample, the maximum as an integer maximum of bit patterns (order-free)
//   lim_init_kernel   the statistics records as a row without a sample over the ceiling has them
//   lim_gain_kernel   a workgroup per tile: x over the tile and 2 L + 6 either side in LDS, r from it; a tile whose r is all 1
//                     ends there (its gains are 1: nothing is written).  Else the sliding minimum by doubling between two
//                     LDS arrays (log2(2 L + 1) passes), the mean as 2 L + 1 additions per sample from LDS in ascending order,
//                     and the limited samples of the tile into the workspace copy; the tile's flag is raised
//   lim_copy_kernel   the flagged tiles from the workspace copy into the rows: in place, and no tile reads what another wrote
// The lengths travel by value; every loop bound is one of them or a host value of the launch.  No floating-point atomics.
#include "api_internal.h"
#include "limiter_plan.h"

// a tap is a product and a sum (tests/limiter_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct LimLens {
    int n[LIM_UTTS];
};

// the taps of the phases 1 .. 3 (phase 0 is the sample itself)
struct LimCoef {
    double h[(LIM_PHASES - 1) * LIM_TAPS];
};

// The envelope of the sample X[5], X[0 .. 12) being x[i - 5 .. i + 6] with zeros outside the utterance.
__device__ __forceinline__ double lim_envelope(const double* X, const LimCoef& coef, bool os4) {
    const double x = X[LIM_BEFORE];
    if (!isfinite(x)) return 0.0;
    double a = fabs(x);
    if (os4) {
#pragma unroll
        for (int p = 0; p < LIM_PHASES - 1; ++p) {
            double acc = __dmul_rn(coef.h[p * LIM_TAPS], X[0]);
#pragma unroll
            for (int k = 1; k < LIM_TAPS; ++k) acc = __dadd_rn(acc, __dmul_rn(coef.h[p * LIM_TAPS + k], X[k]));
            const double v = fabs(acc);
            if (isfinite(acc) && v > a) a = v;
        }
    }
    return a;
}

// X[k] = x[first + k] for k < count, zero outside 0 .. n - 1
__device__ __forceinline__ void lim_load(double* X, const float* __restrict__ x, int n, long long first, int count) {
    for (int k = threadIdx.x; k < count; k += LIM_LANES) {
        const long long j = first + k;
        X[k] = (j >= 0 && j < n) ? (double)x[j] : 0.0;
    }
}

// the largest of the wave's non-negative doubles, in every lane
__device__ __forceinline__ double lim_wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        if (o > v) v = o;
    }
    return v;
}

// peaks[b] (true peak) and sample_peaks[b] (or null): bit patterns of non-negative doubles, zeroed before
__global__ __launch_bounds__(LIM_LANES) void lim_peak_kernel(const float* __restrict__ wav, size_t row, LimLens lens, LimCoef coef,
                                                             unsigned long long* __restrict__ peaks, unsigned long long* __restrict__ sample_peaks) {
    __shared__ double X[LIM_TILE + LIM_BEFORE + LIM_AFTER];
    const int b = blockIdx.y;
    const int n = lens.n[b];
    const long long first = (long long)blockIdx.x * LIM_TILE;
    if (first >= n) return;
    const float* x = wav + (size_t)b * row;
    lim_load(X, x, n, first - LIM_BEFORE, LIM_TILE + LIM_BEFORE + LIM_AFTER);
    __syncthreads();
    double tp = 0.0, sp = 0.0;
    for (int k = threadIdx.x; k < LIM_TILE; k += LIM_LANES) {
        if (first + k < n) {
            const double a = lim_envelope(X + k, coef, true);
            const double s = isfinite(X[k + LIM_BEFORE]) ? fabs(X[k + LIM_BEFORE]) : 0.0;
            if (a > tp) tp = a;
            if (s > sp) sp = s;
        }
    }
    tp = lim_wave_max(tp);
    sp = lim_wave_max(sp);
    if ((threadIdx.x & 63) == 0) {
        if (tp > 0.0) atomicMax(peaks + b, (unsigned long long)__double_as_longlong(tp));
        if (sample_peaks && sp > 0.0) atomicMax(sample_peaks + b, (unsigned long long)__double_as_longlong(sp));
    }
}

__global__ void lim_init_kernel(tts_limit_stats_t* __restrict__ stats, int nb) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    stats[b].over = 0;
    stats[b].limited = 0;
    stats[b].min_gain = 1.0;
}

// wav: the first utterance of the launch, rows `row` floats apart, read only; out: the workspace copy, laid out alike; flags:
// [utterance][flags_row], zeroed before; stats: the launch's records, initialised before.
__global__ __launch_bounds__(LIM_LANES) void lim_gain_kernel(const float* __restrict__ wav, size_t row, LimLens lens, LimCoef coef, double c, float cf,
                                                             int L, int os4, float* __restrict__ out, int* __restrict__ flags, size_t flags_row,
                                                             tts_limit_stats_t* __restrict__ stats) {
    extern __shared__ __align__(16) double lim_lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = lens.n[b];
    const long long first = (long long)blockIdx.x * LIM_TILE;
    if (first >= n) return;
    const float* x = wav + (size_t)b * row;
    const int xc = lim_x_count(L), rc = lim_r_count(L);
    double* X = lim_lds;
    double* R = X + xc;
    double* S = R + rc;
    lim_load(X, x, n, lim_x_first(first, L), xc);
    __syncthreads();
    // r over the tile and 2 L either side; 1 outside the utterance, which no minimum notices (every window holds its own r <= 1)
    const long long rf = lim_r_first(first, L);
    int any = 0;
    for (int k = tid; k < rc; k += LIM_LANES) {
        const long long j = rf + k;
        double r = 1.0;
        if (j >= 0 && j < n) {
            const double a = lim_envelope(X + k, coef, os4 != 0);
            if (a > c) r = __ddiv_rn(c, a);
        }
        R[k] = r;
        any |= r < 1.0;
    }
    if (!__syncthreads_or(any)) return;   // every gain of the tile is 1: its samples stay as they are (also: R is written)

    // The minimum over [k, k + W), W = 2 L + 1, by doubling: R -> S -> X -> S -> ... (x is no longer needed in LDS, r is)
    const int W = 2 * L + 1, steps = lim_min_steps(W), span = lim_min_span(W);
    const double* cur = R;
    for (int t = 0; t < steps; ++t) {
        double* dst = cur == S ? X : S;
        const int off = 1 << t;
        for (int k = tid; k < rc; k += LIM_LANES) {
            const double u = cur[k], v = k + off < rc ? cur[k + off] : 1.0;
            dst[k] = v < u ? v : u;
        }
        __syncthreads();
        cur = dst;
    }
    const double* M = R;   // M[q] = min r over [q, q + W): m[i] = M[i - first + L]
    if (steps) {
        double* dst = cur == S ? X : S;
        const int mc = LIM_TILE + 2 * L;
        for (int k = tid; k < mc; k += LIM_LANES) {
            const double u = cur[k], v = cur[k + W - span];
            dst[k] = v < u ? v : u;
        }
        __syncthreads();
        M = dst;
    }

    int over = 0, limited = 0;
    double lowest = 1.0;
    float* y = out + (size_t)b * row;
    // The sums m[cl(i - L)] + ... + m[cl(i + L)] in ascending order, m[j] = M[j - first + L].  Where no window of the tile leaves
    // the utterance (uniform) a lane runs the sums of its LIM_PER_LANE samples side by side: each is a chain of dependent
    // additions, and the LDS of a workgroup leaves a SIMD two waves to hide them behind.
    const bool inside = first - L >= 0 && first + LIM_TILE + L <= n;
    double sums[LIM_PER_LANE] = {};
    if (inside) {
        const double* w = M + tid;
#pragma unroll
        for (int u = 0; u < LIM_PER_LANE; ++u) sums[u] = w[u * LIM_LANES];
        for (int j = 1; j < W; ++j) {
#pragma unroll
            for (int u = 0; u < LIM_PER_LANE; ++u) sums[u] = __dadd_rn(sums[u], w[u * LIM_LANES + j]);
        }
    }
#pragma unroll
    for (int u = 0; u < LIM_PER_LANE; ++u) {
        const int k = tid + u * LIM_LANES;
        const long long i = first + k;
        if (i >= n) break;
        double acc = sums[u];
        if (!inside) {
            long long j = i - L;
            acc = M[(j < 0 ? 0 : j) - first + L];
            for (++j; j <= i + L; ++j) acc = __dadd_rn(acc, M[(j < 0 ? 0 : j >= n ? n - 1 : j) - first + L]);
        }
        const double s = __ddiv_rn(acc, (double)W);
        const double r = R[k + 2 * L];
        const double g = s < r ? s : r;
        const float xi = x[i];
        float o = xi;
        if (isfinite(xi)) {
            over += r < 1.0;
            if (g < 1.0) {
                ++limited;
                if (g < lowest) lowest = g;
                const float v = fabsf((float)__dmul_rn(g, (double)xi));
                o = copysignf(v < cf ? v : cf, xi);
            }
        }
        y[i] = o;
    }
    if (tid == 0) flags[(size_t)b * flags_row + blockIdx.x] = 1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        over += __shfl_xor(over, off, 64);
        limited += __shfl_xor(limited, off, 64);
        const double o = __shfl_xor(lowest, off, 64);
        if (o < lowest) lowest = o;
    }
    if ((tid & 63) == 0) {
        if (over) atomicAdd(&stats[b].over, over);
        if (limited) atomicAdd(&stats[b].limited, limited);
        // (positive doubles order as their bit patterns)
        if (lowest < 1.0) atomicMin(reinterpret_cast<unsigned long long*>(&stats[b].min_gain), (unsigned long long)__double_as_longlong(lowest));
    }
}

__global__ __launch_bounds__(LIM_LANES) void lim_copy_kernel(float* __restrict__ wav, size_t row, LimLens lens, const float* __restrict__ out,
                                                             const int* __restrict__ flags, size_t flags_row) {
    const int b = blockIdx.y;
    const int n = lens.n[b];
    const long long first = (long long)blockIdx.x * LIM_TILE;
    if (first >= n || !flags[(size_t)b * flags_row + blockIdx.x]) return;
    float* x = wav + (size_t)b * row;
    const float* y = out + (size_t)b * row;
    for (int k = threadIdx.x; k < LIM_TILE; k += LIM_LANES) {
        const long long i = first + k;
        if (i < n) x[i] = y[i];
    }
}

}  // namespace tts

namespace tts_api {

static LimCoef lim_coef() {
    const LimTaps t = lim_taps();
    LimCoef c;
    for (int i = 0; i < (LIM_PHASES - 1) * LIM_TAPS; ++i) c.h[i] = t.h[LIM_TAPS + i];
    return c;
}

// The workspaces of a tts_limit call on B rows of N samples.
int limiter_scratch(tts_handle_t h, int B, int N, LimScratch* s) {
    WS(h, "lim.out", float, (size_t)B * N, out);
    WS(h, "lim.flags", int, (size_t)B * lim_tiles(N), flags);
    WS(h, "lim.stats", tts_limit_stats_t, (size_t)B, st);
    *s = LimScratch{out, flags, st};
    return TTS_OK;
}

// On h->stream; everything has been checked (limiter_check).
int limiter_impl(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, double ceiling, int lookahead, int oversample,
                 tts_limit_stats_t* stats) {
    LimScratch s;
    const int rc = limiter_scratch(h, B, N, &s);
    if (rc) return rc;
    const size_t flags_row = (size_t)lim_tiles(N);   // a flag per tile of a row
    const LimCoef coef = lim_coef();
    const float cf = lim_ceiling_float(ceiling);
    const size_t lds = lim_lds_bytes(lookahead);
    if (lds > 64 * 1024)   // (what this call asks for, not all 160 KB: the block-wide vote keeps a few bytes of its own)
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&lim_gain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    tts_limit_stats_t* st = stats ? stats : s.stats;
    ProfScope ps(h, ST_LIMITER, (int64_t)length_chunks(B, LIM_UTTS) * 3 + 1);
    HIPCHK(h, hipMemsetAsync(s.flags, 0, (size_t)B * flags_row * sizeof(int), h->stream));
    for (int b0 = 0; b0 < B; b0 += LIM_UTTS) {
        const int nb = std::min(LIM_UTTS, B - b0);
        LimLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        const dim3 grid((unsigned)lim_tiles(longest), nb);
        float* pw = wav + (size_t)b0 * N;
        float* po = s.out + (size_t)b0 * N;
        int* pf = s.flags + (size_t)b0 * flags_row;
        hipLaunchKernelGGL(lim_init_kernel, dim3(1), dim3(LIM_UTTS), 0, h->stream, st + b0, nb);
        hipLaunchKernelGGL(lim_gain_kernel, grid, dim3(LIM_LANES), lds, h->stream, pw, (size_t)N, lens, coef, ceiling, cf, lookahead,
                           oversample == 4 ? 1 : 0, po, pf, flags_row, st + b0);
        hipLaunchKernelGGL(lim_copy_kernel, grid, dim3(LIM_LANES), 0, h->stream, pw, (size_t)N, lens, po, pf, flags_row);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

static int true_peak_impl(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, double* true_peak, double* sample_peak) {
    const LimCoef coef = lim_coef();
    ProfScope ps(h, ST_LIMITER, (int64_t)length_chunks(B, LIM_UTTS) + (sample_peak ? 2 : 1));
    HIPCHK(h, hipMemsetAsync(true_peak, 0, (size_t)B * sizeof(double), h->stream));
    if (sample_peak) HIPCHK(h, hipMemsetAsync(sample_peak, 0, (size_t)B * sizeof(double), h->stream));
    for (int b0 = 0; b0 < B; b0 += LIM_UTTS) {
        const int nb = std::min(LIM_UTTS, B - b0);
        LimLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        hipLaunchKernelGGL(lim_peak_kernel, dim3((unsigned)lim_tiles(longest), nb), dim3(LIM_LANES), 0, h->stream, wav + (size_t)b0 * N, (size_t)N, lens,
                           coef, reinterpret_cast<unsigned long long*>(true_peak) + b0,
                           sample_peak ? reinterpret_cast<unsigned long long*>(sample_peak) + b0 : nullptr);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_true_peak_filter(double coeffs[48]) {
    if (!coeffs) return TTS_ERR_INVALID;
    const LimTaps t = lim_taps();
    for (int i = 0; i < LIM_PHASES * LIM_TAPS; ++i) coeffs[i] = t.h[i];
    return TTS_OK;
}

int tts_limit_max_lookahead(void) { return LIM_MAX_LOOKAHEAD; }

int tts_true_peak(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, double* true_peak, double* sample_peak) {
    DeviceScope dev_scope(h);
    std::string why = limiter_check(wav && true_peak, B, N, n_samples, false, 1.0, 0, 1);
    if (why.empty() && (((reinterpret_cast<uintptr_t>(true_peak) | reinterpret_cast<uintptr_t>(sample_peak)) & 7) || (reinterpret_cast<uintptr_t>(wav) & 3)))
        why = "true_peak and sample_peak must be 8-byte aligned, wav 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "true_peak: " + why);
    if (!h) return TTS_ERR_INVALID;
    return true_peak_impl(h, wav, B, N, n_samples, true_peak, sample_peak);
}

int tts_limit(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, double ceiling, int lookahead, int oversample,
              tts_limit_stats_t* stats) {
    DeviceScope dev_scope(h);
    std::string why = limiter_check(wav != nullptr, B, N, n_samples, true, ceiling, lookahead, oversample);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(stats) & 7) || (reinterpret_cast<uintptr_t>(wav) & 3)))
        why = "stats must be 8-byte aligned, wav 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "limit: " + why);
    if (!h) return TTS_ERR_INVALID;
    return limiter_impl(h, wav, B, N, n_samples, ceiling, lookahead, oversample, stats);
}

int tts_set_limiter(tts_handle_t h, int enabled, double ceiling, int lookahead, int oversample) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled) {
        const std::string why = limiter_check(true, 1, 1, nullptr, true, ceiling, lookahead, oversample);
        if (!why.empty()) return fail(h, TTS_ERR_INVALID, "set_limiter: " + why);
        h->settings.lim.ceiling = ceiling;
        h->settings.lim.lookahead = lookahead;
        h->settings.lim.oversample = oversample;
    }
    h->settings.lim.enabled = enabled != 0;
    return TTS_OK;
}

}  // extern "C"
