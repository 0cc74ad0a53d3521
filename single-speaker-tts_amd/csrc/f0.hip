// F0 tracking: YIN (de Cheveigne and Kawahara 2002, steps 2 to 5) on batches of waveforms, and the F0 / voicing errors of two
// tracks along a DTW path (audio/metrics.py).  No reference counterpart.  include/sstts_hip.h has the definition in full; every
// operation is an individually rounded IEEE double operation, so the results are the bits of tests/f0_oracle.py.
//
// f0_kernel: a workgroup owns `frames` consecutive frames of one utterance (f0_plan.h).  It stages their common span in LDS as
// doubles once -- samples outside [0, n_b) are 0.0 and never read -- and gives every lane the lags tau = 1 + lane + s * F0_LANES.
// For a frame a lane walks j = 0 .. W - 1 with x(s0 + j) as a broadcast read and x(s0 + j + tau) as a consecutive 8-byte read
// (conflict-free), three double operations per lag and j.  The running sum c of the normalisation is sequential by contract: lane
// f walks the chain of frame f, so the chains of a group run side by side in one wave (rows an odd number of doubles apart lie on
// different banks); the quotients are then taken by all lanes.  The threshold, the argmin and the descent are first-index
// reductions of a wave per frame: a strided pass over [tau_min, tau_max] and shuffles.  No atomics; every loop bound is a host
// value that travelled in the launch.
//
// f0_compare_kernel: one wave per utterance walks the `rows` rows of a tts_dtw path in chunks of 64.  A lane takes the terms of
// one step; the two sums are then added in step order by every lane alike (a skipped step adds +0.0, which changes no bit of a
// sum that starts at +0.0 and only ever receives squares or NaN).
#include "api_internal.h"
#include "f0_plan.h"

// s = s + u * u is a product and a sum (tests/f0_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct F0Lens {
    int n[F0_UTTS];
};

// wav, f0 and ap point at the first utterance of the launch; row: floats between two utterances of wav; T: frames of a row of
// f0 / ap; frames: frames per workgroup.  Dynamic LDS: f0_lds_bytes(W, tau_max, hop, frames).
template <int SLOTS>
__global__ __launch_bounds__(F0_LANES) void f0_kernel(const float* __restrict__ wav, size_t row, F0Lens lens, int T, int hop, int W, int tau_min,
                                                      int tau_max, int frames, double threshold, double sampling_rate, float* __restrict__ f0,
                                                      float* __restrict__ ap) {
    extern __shared__ __align__(16) double f0_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n = lens.n[b];
    const int t0 = blockIdx.x * frames;
    const int nf = min(frames, T - t0);                            // frames of this group that exist in the output
    const int nv = max(0, min(nf, f0_frames(n, hop) - t0));        // ... of which the first nv belong to the utterance
    float* out_f0 = f0 + (size_t)b * T + t0;
    float* out_ap = ap ? ap + (size_t)b * T + t0 : nullptr;
    for (int f = nv + tid; f < nf; f += F0_LANES) {                // padding frames
        out_f0[f] = 0.f;
        if (out_ap) out_ap[f] = 0.f;
    }
    if (nv == 0) return;   // (uniform)

    const int stride = f0_row_stride(tau_max);
    const int span = W + tau_max + (nv - 1) * hop;                 // <= f0_span(W, tau_max, hop, frames): what the launch asked for
    double* sx = f0_lds;
    double* sq = f0_lds + f0_span(W, tau_max, hop, frames);        // [frames][stride]: d, then q
    double* sc = sq + (size_t)frames * stride;                     // [frames][stride]: the running sums c
    const float* x = wav + (size_t)b * row;
    const long long g0 = f0_first_sample(t0, hop, W, tau_max);
    for (int i = tid; i < span; i += F0_LANES) {
        const long long at = g0 + i;
        sx[i] = (at >= 0 && at < n) ? (double)x[at] : 0.0;
    }
    __syncthreads();

    // ---- the difference function
    int lag[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) lag[s] = min(1 + tid + s * F0_LANES, tau_max);   // (a lane beyond tau_max repeats the last lag, and stores nothing)
    for (int f = 0; f < nv; ++f) {
        const double* xf = sx + (size_t)f * hop;
        double acc[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) acc[s] = 0.0;
        for (int j = 0; j < W; ++j) {
            const double xb = xf[j];
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const double u = __dsub_rn(xb, xf[j + lag[s]]);
                acc[s] = __dadd_rn(acc[s], __dmul_rn(u, u));
            }
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (1 + tid + s * F0_LANES <= tau_max) sq[(size_t)f * stride + lag[s]] = acc[s];
    }
    __syncthreads();

    // ---- the normalisation: c = c + d[tau], one chain per frame
    if (tid < nv) {
        const double* d = sq + (size_t)tid * stride;
        double* cs = sc + (size_t)tid * stride;
        double c = 0.0;
        for (int tau = 1; tau <= tau_max; ++tau) {
            c = __dadd_rn(c, d[tau]);
            cs[tau] = c;
        }
    }
    __syncthreads();
    for (int i = tid; i < nv * tau_max; i += F0_LANES) {
        const int f = i / tau_max, tau = 1 + i % tau_max;
        const double d = sq[(size_t)f * stride + tau], c = sc[(size_t)f * stride + tau];
        sq[(size_t)f * stride + tau] = (c == 0.0) ? 1.0 : __ddiv_rn(__dmul_rn(d, (double)tau), c);
    }
    __syncthreads();

    // ---- the decisions: one wave per frame
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int NONE = 0x7fffffff;
    for (int f = wave; f < nv; f += F0_LANES / 64) {
        const double* q = sq + (size_t)f * stride;
        const double c_last = sc[(size_t)f * stride + tau_max];
        if (!isfinite(c_last)) {   // (uniform in the wave) a NaN or Inf sample in the span
            if (lane == 0) {
                out_f0[f] = __builtin_nanf("");
                if (out_ap) out_ap[f] = __builtin_nanf("");
            }
            continue;
        }
        // the first lag under the threshold, and the first index of the minimum (no q is NaN here: c is finite)
        int first = NONE, bi = NONE;
        double bv = 0.0;
        for (int tau = tau_min + lane; tau <= tau_max; tau += 64) {
            const double v = q[tau];
            if (v < threshold && tau < first) first = tau;
            if (bi == NONE || v < bv) bv = v, bi = tau;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            first = min(first, __shfl_xor(first, off, 64));
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != NONE && (bi == NONE || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        }
        if (first == NONE) {   // unvoiced
            if (lane == 0) {
                out_f0[f] = 0.f;
                if (out_ap) out_ap[f] = (float)q[bi];
            }
            continue;
        }
        // the descent: the first lag at or behind `first` that is the last one or whose successor is not smaller
        int star = NONE;
        for (int tau = tau_min + lane; tau <= tau_max; tau += 64) {
            bool stop = tau == tau_max;
            if (!stop) stop = !(q[tau + 1] < q[tau]);
            if (stop && tau >= first && tau < star) star = tau;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) star = min(star, __shfl_xor(star, off, 64));
        if (lane == 0) {
            double delta = 0.0;
            if (star < tau_max) {
                const double a = q[star - 1], bq = q[star], g = q[star + 1];
                const double den = __dsub_rn(__dadd_rn(a, g), __dadd_rn(bq, bq));
                if (a >= bq && g >= bq && den > 0.0) delta = __ddiv_rn(__dmul_rn(0.5, __dsub_rn(a, g)), den);
            }
            out_f0[f] = (float)__ddiv_rn(sampling_rate, __dadd_rn((double)star, delta));
            if (out_ap) out_ap[f] = (float)q[star];
        }
    }
}

// counts: {steps, both voiced, one voiced, gross pitch errors, NaN steps}; sums: {sum (fa - fb)^2, sum (1200 log2(fa / fb))^2}
__global__ __launch_bounds__(64) void f0_compare_kernel(const float* __restrict__ f0_a, int Ta, const float* __restrict__ f0_b, int Tb,
                                                        const int32_t* __restrict__ path, int rows, int32_t* __restrict__ counts,
                                                        double* __restrict__ sums) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const float* A = f0_a + (size_t)p * Ta;
    const float* Bv = f0_b + (size_t)p * Tb;
    const int32_t* P = path + (size_t)p * rows * 2;
    int cnt[5] = {0, 0, 0, 0, 0};
    double s_hz = 0.0, s_cents = 0.0;
    for (int k0 = 0; k0 < rows; k0 += 64) {
        const int k = k0 + lane;
        double uu = 0.0, zz = 0.0;
        if (k < rows) {
            const int i = P[2 * (size_t)k], j = P[2 * (size_t)k + 1];
            if (i >= 0 && j >= 0 && i < Ta && j < Tb) {   // rows behind the path are (-1, -1)
                const double fa = (double)A[i], fb = (double)Bv[j];
                ++cnt[0];
                if (fa != fa || fb != fb) {
                    ++cnt[4];
                } else if ((fa > 0.0) != (fb > 0.0)) {
                    ++cnt[2];
                } else if (fa > 0.0) {
                    ++cnt[1];
                    const double u = __dsub_rn(fa, fb);
                    uu = __dmul_rn(u, u);
                    if (fabs(u) > __dmul_rn(0.2, fb)) ++cnt[3];
                    const double z = __dmul_rn(1200.0, log2(__ddiv_rn(fa, fb)));
                    zz = __dmul_rn(z, z);
                }
            }
        }
        const int steps = min(64, rows - k0);   // (uniform)
        for (int l = 0; l < steps; ++l) {
            s_hz = __dadd_rn(s_hz, __shfl(uu, l, 64));
            s_cents = __dadd_rn(s_cents, __shfl(zz, l, 64));
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt[c] += __shfl_xor(cnt[c], off, 64);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 5; ++c) counts[(size_t)p * 5 + c] = cnt[c];
        sums[(size_t)p * 2] = s_hz;
        sums[(size_t)p * 2 + 1] = s_cents;
    }
}

}  // namespace tts

namespace tts_api {

template <int SLOTS>
static void f0_launch(tts_handle_t h, dim3 grid, size_t lds, const float* wav, size_t row, const F0Lens& lens, int T, int hop, int W, int tau_min,
                      int tau_max, int frames, double threshold, double sampling_rate, float* f0, float* ap) {
    hipLaunchKernelGGL(f0_kernel<SLOTS>, grid, dim3(F0_LANES), lds, h->stream, wav, row, lens, T, hop, W, tau_min, tau_max, frames, threshold,
                       sampling_rate, f0, ap);
}

// On h->stream; everything has been checked (f0_check).
static int f0_impl(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, double sampling_rate, int hop, int W, int tau_min,
                   int tau_max, double threshold, float* f0, float* ap) {
    const int T = f0_frames(N, hop);
    const int frames = f0_group_frames(W, tau_max, hop);
    const size_t lds = f0_lds_bytes(W, tau_max, hop, frames);
    const int groups = f0_groups(T, frames);
    ProfScope ps(h, ST_F0, length_chunks(B, F0_UTTS));
    for (int b0 = 0; b0 < B; b0 += F0_UTTS) {
        const int nb = std::min(F0_UTTS, B - b0);
        F0Lens lens;
        fill_lengths(lens.n, n_samples, b0, nb, N);
        const float* pw = wav + (size_t)b0 * N;
        float* pf = f0 + (size_t)b0 * T;
        float* pa = ap ? ap + (size_t)b0 * T : nullptr;
        const dim3 grid(groups, nb);
        switch (f0_slots(tau_max)) {
            case 1: f0_launch<1>(h, grid, lds, pw, (size_t)N, lens, T, hop, W, tau_min, tau_max, frames, threshold, sampling_rate, pf, pa); break;
            case 2: f0_launch<2>(h, grid, lds, pw, (size_t)N, lens, T, hop, W, tau_min, tau_max, frames, threshold, sampling_rate, pf, pa); break;
            case 3: f0_launch<3>(h, grid, lds, pw, (size_t)N, lens, T, hop, W, tau_min, tau_max, frames, threshold, sampling_rate, pf, pa); break;
            default: f0_launch<4>(h, grid, lds, pw, (size_t)N, lens, T, hop, W, tau_min, tau_max, frames, threshold, sampling_rate, pf, pa); break;
        }
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_f0(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, double sampling_rate, int hop, int W, int tau_min, int tau_max,
           double threshold, float* f0, float* aperiodicity) {
    DeviceScope dev_scope(h);
    bool unsupported = false;
    std::string why = f0_check(wav && f0, B, N, n_samples, sampling_rate, hop, W, tau_min, tau_max, threshold, &unsupported);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(f0) | reinterpret_cast<uintptr_t>(aperiodicity)) & 3))
        why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "f0: " + why);
    if (!h) return TTS_ERR_INVALID;
    return f0_impl(h, wav, B, N, n_samples, sampling_rate, hop, W, tau_min, tau_max, threshold, f0, aperiodicity);
}

int tts_f0_compare(tts_handle_t h, const float* f0_a, int Ta, const float* f0_b, int Tb, const int32_t* path, int rows, int B, int32_t* counts,
                   double* sums) {
    DeviceScope dev_scope(h);
    std::string why = f0_compare_check(f0_a && f0_b && path && counts && sums, Ta, Tb, rows, B);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(sums) & 7) || ((reinterpret_cast<uintptr_t>(f0_a) | reinterpret_cast<uintptr_t>(f0_b) |
                                                                      reinterpret_cast<uintptr_t>(path) | reinterpret_cast<uintptr_t>(counts)) & 3)))
        why = "sums must be 8-byte aligned, the other buffers 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "f0_compare: " + why);
    if (!h) return TTS_ERR_INVALID;
    ProfScope ps(h, ST_F0, 1);
    hipLaunchKernelGGL(f0_compare_kernel, dim3(B), dim3(64), 0, h->stream, f0_a, Ta, f0_b, Tb, path, rows, counts, sums);
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}

int tts_f0_frames(int n, int hop) { return (n < 0 || hop < 1) ? 0 : f0_frames(n, hop); }

int tts_f0_max_window(void) { return F0_MAX_WINDOW; }

int tts_f0_max_lag(void) { return F0_MAX_LAG; }

}  // extern "C"
