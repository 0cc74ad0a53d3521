// Band-limited resampling: librosa 0.6 resample(..., res_type='kaiser_best') = resampy 0.2 resample_f with the 'kaiser_best'
// windowed sinc, the second half of the reference's pitch_shift (audio/effects.py:9-43) and what load_wav(sampling_rate=...)
// runs.  For output sample t of an utterance of n_in samples, rho = target rate / source rate (resample_plan.h):
//   tr = t / rho, m = (int)tr, frac = scale (tr - m);   f = 512 frac, off = (int)f, eta = f - off
//   y  = sum_i (win[off + i step] + eta delta[off + i step]) x[m - i]            i < min(m + 1, (32769 - off) / step)
//      + the same with frac = scale - frac on x[m + 1 + k]                        k < min(n_in - m - 1, (32769 - off) / step)
// in double, rounded once to float32.  The index arithmetic is rounded operation by operation (no contraction: the file is built
// with -ffp-contract=off); the weights and the sum use explicit FMAs.
//
// Output t of EVERY utterance of a batch has the same m, off and eta, so a thread computes a tap's weight once and applies it to
// RS_U utterances: the table is then read once per RS_U taps.  A workgroup takes RS_TILE consecutive outputs of RS_U
// utterances; it stages the input samples their windows cover in LDS, interleaved by utterance ([sample][RS_U]: a tap's RS_U
// samples are one or two 16-byte reads), with 0.0 for every sample outside [0, n_in) -- such a sample is never fetched, and a
// product with 0.0 leaves a sum's bits alone, so the wings need no cut at the signal's ends.  The taps walk the per-ratio
// phase-major copy of the table ([off][i] pairs {win, delta}, 16 bytes per tap, contiguous per lane, rows of whole cache
// lines), which is built once per ratio and kept on the handle: about 0.5 MiB, read out of L2.
// The sum of an utterance is taken in the same order whatever RS_U is and wherever the utterance sits: the same bits in every
// batch.  No atomics.  The lengths travel by value in the launch, RS_CHUNK utterances per launch.
#include "api_internal.h"
#include "resample_plan.h"

#pragma clang fp contract(off)

namespace tts {

constexpr int RS_TILE = 256;    // outputs per workgroup, one per thread
constexpr int RS_CHUNK = 64;    // utterances whose lengths one launch carries
constexpr int RS_U = 8;         // utterances a thread applies a weight to (the groups of a chunk; the rest go one by one)

struct ResampleLens {
    int n_in[RS_CHUNK];    // samples of the utterance that may be read
    int keep[RS_CHUNK];    // computed samples its row holds; zeros behind them
};

// the samples a workgroup stages, at most: the windows of RS_TILE outputs
inline int resample_span_max(const ResampleConsts& c) { return (int)((double)(RS_TILE - 1) * c.inc) + 2 + 2 * c.taps_max; }

template <int U>
__device__ __forceinline__ void rs_wing(const double2* __restrict__ trow, int cnt, double eta, const float* xp, int dir, double (&acc)[U]) {
#pragma unroll 8
    for (int i = 0; i < cnt; ++i) {
        const double2 wd = trow[i];
        const double w = fma(eta, wd.y, wd.x);
        const float* p = xp + (ptrdiff_t)dir * i * U;
        if constexpr (U % 4 == 0) {
#pragma unroll
            for (int q = 0; q < U / 4; ++q) {
                const float4 v = reinterpret_cast<const float4*>(p)[q];
                acc[4 * q + 0] = fma(w, (double)v.x, acc[4 * q + 0]);
                acc[4 * q + 1] = fma(w, (double)v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fma(w, (double)v.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fma(w, (double)v.w, acc[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = fma(w, (double)p[u], acc[u]);
        }
    }
}

// x [..][n] -> out [..][N_out] for the utterances b_first + blockIdx.y * U + {0 .. U - 1} of the launch's chunk.
template <int U>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const float* __restrict__ x, float* __restrict__ out, ResampleLens lens, int b_first,
                                                           int n, int N_out, double inc, double scale, int step, int row, int taps_max,
                                                           const double2* __restrict__ tab) {
    extern __shared__ __align__(16) float rs_xs[];   // [span][U]
    const int b0 = b_first + (int)blockIdx.y * U;
    const long long t0 = (long long)blockIdx.x * RS_TILE;
    const long long t = t0 + threadIdx.x;
    int keep_max = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) keep_max = max(keep_max, lens.keep[b0 + u]);
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0;
    if (t0 < keep_max) {   // (uniform over the workgroup; otherwise the tile is zeros only)
        const long long t_last = min(t0 + RS_TILE - 1, (long long)keep_max - 1);
        const long long m_first = (long long)((double)t0 * inc), m_last = (long long)((double)t_last * inc);
        const long long lo = m_first - (taps_max - 1);
        const int span = (int)(m_last - m_first) + 2 * taps_max;
        for (int idx = threadIdx.x; idx < span; idx += RS_TILE) {
            const long long g = lo + idx;
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = (g >= 0 && g < lens.n_in[b0 + u]) ? x[(size_t)(b0 + u) * n + g] : 0.f;
            if constexpr (U % 4 == 0) {
#pragma unroll
                for (int q = 0; q < U / 4; ++q)
                    reinterpret_cast<float4*>(rs_xs + (size_t)idx * U)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) rs_xs[(size_t)idx * U + u] = v[u];
            }
        }
        __syncthreads();
        if (t <= t_last) {
            const double tr = (double)t * inc;
            const long long m = (long long)tr;
            double frac = scale * (tr - (double)m);
            const int at = (int)(m - lo);   // m in the staged samples: taps_max - 1 <= at, at + taps_max < span
            {
                const double f = frac * (double)RS_NUM_TABLE;
                const int off = (int)f;
                const double eta = f - (double)off;
                rs_wing<U>(tab + (size_t)off * row, (RS_NWIN - off) / step, eta, rs_xs + (size_t)at * U, -1, acc);
            }
            {
                frac = scale - frac;
                const double f = frac * (double)RS_NUM_TABLE;
                const int off = (int)f;
                const double eta = f - (double)off;
                rs_wing<U>(tab + (size_t)off * row, (RS_NWIN - off) / step, eta, rs_xs + (size_t)(at + 1) * U, 1, acc);
            }
        }
    }
    if (t < N_out) {
#pragma unroll
        for (int u = 0; u < U; ++u) out[(size_t)(b0 + u) * N_out + t] = t < lens.keep[b0 + u] ? (float)acc[u] : 0.f;
    }
}

}  // namespace tts

namespace tts_api {

// The phase-major table of a ratio on the device: built on first use (a synchronous upload, once per ratio) and kept on the
// handle.  Ratios of 1 and above share one table (scale = 1); below 1 the window carries the ratio.
int resample_table(tts_handle_t h, double rho, const double** tab) {
    auto& rs = h->rs;
    const ResampleConsts c = resample_consts(rho);
    uint64_t key = 0;
    std::memcpy(&key, &c.scale, sizeof(key));
    auto it = rs.tabs.find(key);
    if (it == rs.tabs.end()) {
        if (rs.tabs.size() >= 32) {   // (a caller sweeping ratios: start over, behind everything that reads the old tables)
            const int rc = sync_all(h);
            if (rc) return rc;
            for (auto& kv : rs.tabs) hipFree(kv.second);
            rs.tabs.clear();
        }
        if (rs.base.empty()) rs.base = resample_half_window();
        const std::vector<double> host = resample_phase_table(rs.base, rho, c);
        double* dev = nullptr;
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&dev), host.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(dev);
            HIPCHK(h, e);
        }
        it = rs.tabs.emplace(key, dev).first;
    }
    *tab = it->second;
    return TTS_OK;
}

// On h->stream.  n_samples: HOST lengths or null (all n); keep_cap: HOST, or null -- row b holds at most keep_cap[b] computed
// samples (the call pipeline's rows end where the un-shifted call's do).  Everything has been checked (resample_check).
int resample_impl(tts_handle_t h, const float* wav, int B, int n, const int32_t* n_samples, double rho, int N_out, const int32_t* keep_cap,
                  float* out) {
    const double* tab = nullptr;
    int rc = resample_table(h, rho, &tab);
    if (rc) return rc;
    const ResampleConsts c = resample_consts(rho);
    const int span_max = resample_span_max(c);
    int n_launches = 0;
    for (int b0 = 0; b0 < B; b0 += RS_CHUNK) {
        const int nb = std::min(RS_CHUNK, B - b0);
        n_launches += (nb / RS_U > 0) + (nb % RS_U > 0);
    }
    ProfScope ps(h, ST_RESAMPLE, n_launches);
    const unsigned tiles = (unsigned)(((long long)N_out + RS_TILE - 1) / RS_TILE);
    const double2* tab2 = reinterpret_cast<const double2*>(tab);
    for (int b0 = 0; b0 < B; b0 += RS_CHUNK) {
        const int nb = std::min(RS_CHUNK, B - b0);
        ResampleLens lens = {};
        fill_lengths(lens.n_in, n_samples, b0, nb, n);
        for (int b = 0; b < nb; ++b) {
            long long keep = std::min<long long>(resampled_valid(lens.n_in[b], rho), N_out);
            if (keep_cap) keep = std::min<long long>(keep, std::max(0, keep_cap[b0 + b]));
            lens.keep[b] = (int)keep;
        }
        const float* src = wav + (size_t)b0 * n;
        float* dst = out + (size_t)b0 * N_out;
        const int groups = nb / RS_U, rest = nb % RS_U;
        if (groups)
            hipLaunchKernelGGL(resample_kernel<RS_U>, dim3(tiles, groups), dim3(RS_TILE), (size_t)span_max * RS_U * sizeof(float), h->stream, src,
                               dst, lens, 0, n, N_out, c.inc, c.scale, c.step, c.row, c.taps_max, tab2);
        if (rest)
            hipLaunchKernelGGL(resample_kernel<1>, dim3(tiles, rest), dim3(RS_TILE), (size_t)span_max * sizeof(float), h->stream, src, dst, lens,
                               groups * RS_U, n, N_out, c.inc, c.scale, c.step, c.row, c.taps_max, tab2);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

void resample_release(tts_handle_t h) {
    for (auto& kv : h->rs.tabs) hipFree(kv.second);
    h->rs.tabs.clear();
}

}  // namespace tts_api

extern "C" {

int tts_resampled_length(int n, double ratio, int* out) {
    if (!out || n < 1 || !resample_ratio_ok(ratio)) return TTS_ERR_INVALID;
    const long long m = resampled_length(n, ratio);
    if (m > INT32_MAX) return TTS_ERR_INVALID;
    *out = (int)m;
    return TTS_OK;
}

int tts_resample(tts_handle_t h, const float* wav, int B, int n, const int32_t* n_samples, double ratio, int N_out, float* out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const std::string why = resample_check(wav && out, B, n, n_samples, ratio, N_out);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "resample: " + why);
    return resample_impl(h, wav, B, n, n_samples, ratio, N_out, nullptr, out);
}

}  // extern "C"
