// Dataset features on the GPU: the silence trim and the feature pass of reference datasets/lj_speech.py:106-156 (load_audio)
// for a RAGGED batch of recordings (gfx950).
//
//   trim_mse_kernel      one wave per (recording, trim frame) item: mean square of the reflect-padded frame in float64
//   trim_bounds_kernel   one workgroup per recording: librosa 0.6 effects.trim's decision on those (float64), -> {start, end}
//   feat2048_kernel      n_fft 2048: one wave per (recording, output frame) item, the one-wave FFT of griffin_lim.hip's
//                        stft_kernel (fft_wave.h), then |X| -> linear dB row, HTK mel of |X| -> mel dB row
//   feat_generic_kernel  any power-of-two n_fft (256 .. 4096): one workgroup per item, the LDS FFT of griffin_lim_generic.hip
//                        (fft_lds.h), same rows
//
// Work is dealt from flat item lists: the host uploads one small descriptor per recording (where its samples and output rows
// start) and a kernel finds an item's recording by binary search over those starts.  So a batch takes two trim launches and one
// feature launch whatever B and the lengths are, and an item's arithmetic depends on its recording alone: a recording's rows
// are the same bits at any position of any batch.  Output rows are written time-major straight into the caller's ragged
// buffers ([sum T_pad][n_mels], [sum T_pad][F]): the reference's (T_pad / r, F r) arrays are reshapes of (T_pad, F), and its
// zero reduction padding (applied after normalisation) is written by the same launch.
//
// No packed-f32 instructions: the file is built with -fno-slp-vectorize like its neighbours (build.py) and takes fft_wave.h in
// its scalar form (FFT_WAVE_SCALAR).  With the packed helpers the 2048 path gave other bits for 32 of 160 recordings while MFMA
// GEMM waves of another handle shared the compute units (tests/test_gpu_features.py, the fault griffin_lim_generic.hip met).
#include "api_internal.h"
#include "fft_lds.h"
#define FFT_WAVE_SCALAR
#include "fft_wave.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace tts {

#define FEAT_NW 8                 // waves per workgroup of feat2048_kernel
#define FEAT_THREADS (FEAT_NW * 64)
#define FEAT_GTHREADS 256         // feat_generic_kernel
#define TRIM_THREADS 256

struct TrimDesc {                 // one recording of tts_trim_bounds
    long long off;                // first sample in wav
    long long fr0;                // first trim-frame item
    int n;                        // samples
    int pad;
};
struct FeatDesc {                 // one recording of tts_extract_features
    long long start;              // first sample of the analysed segment in wav
    long long row0;               // first output row
    int len;                      // samples of the segment
    int Tf;                       // frames with data (rows Tf .. T_pad - 1 are zero)
};

// index of the last descriptor whose `first` is <= g (the firsts increase strictly)
template <typename D, typename F>
__device__ __forceinline__ int find_item(const D* __restrict__ d, int B, long long g, F first) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(d[mid]) <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// numpy's max: a NaN operand gives the NaN (fmax would return the other operand)
__device__ __forceinline__ double max_keep_nan(double a, double b) { return a != a ? a : (b != b ? b : fmax(a, b)); }

__device__ __forceinline__ int reflect_index(long long i, int n) {   // numpy.pad(mode='reflect'), one bounce (pad < n)
    i = i < 0 ? -i : i;
    return (int)(i >= n ? 2 * (long long)(n - 1) - i : i);
}

// magnitude_to_decibel (float64 log, as tts_db_convert mode 0) and, when norm, normalize_decibel (as mode 2).  A NaN
// magnitude stays a NaN in both forms, as np.maximum and np.clip leave it (fmaxf / fminf alone would return 1e-5 and the
// clip edge: "Non-finite values" in include/sstts_hip.h); every other x takes the fmaxf / fminf path bit for bit.
__device__ __forceinline__ float feat_db(float x, int norm, float ref_db, float range) {
    const float db = (float)(20.0 * log10((double)(x != x ? x : fmaxf(1e-5f, x))));
    return norm ? clip_keep_nan(1.0f + (db - ref_db) / range, 0.f, 1.f) : db;
}

struct FeatArgs {
    const float* wav;
    const FeatDesc* desc;
    int B;
    long long rows;               // sum of T_pad
    const float* window;          // [win]
    int win, hop;
    int n_mels;
    const float* mel_w;           // packed filterbank weights
    const int* mel_band;          // [n_mels][3] {first bin, first weight, end bin}
    int norm;
    float mel_ref, mel_range, lin_ref, lin_range;
    float* mel_out;
    float* lin_out;
};

// ------------------------------------------------------------------------------------------------ trim
__global__ __launch_bounds__(TRIM_THREADS) void trim_mse_kernel(const float* __restrict__ wav, const TrimDesc* __restrict__ d,
                                                               int B, long long items, int L, int H, double* __restrict__ mse) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (TRIM_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= items) return;
    const int b = find_item(d, B, g, [](const TrimDesc& x) { return x.fr0; });
    const TrimDesc r = d[b];
    const long long k = g - r.fr0;
    const float* y = wav + r.off;
    const long long base = k * H - (L >> 1);
    double s = 0.0;
    for (int j = lane; j < L; j += 64) {
        const double v = (double)y[reflect_index(base + j, r.n)];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) mse[g] = s / (double)L;
}

__global__ __launch_bounds__(TRIM_THREADS) void trim_bounds_kernel(const TrimDesc* __restrict__ d, const double* __restrict__ mse,
                                                                  int H, double top_db, long long* __restrict__ bounds) {
    __shared__ double red[TRIM_THREADS];
    __shared__ int first_s, last_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrimDesc r = d[b];
    const int nf = r.n / H + 1;
    const double* m = mse + r.fr0;
    double mx = 0.0;
    for (int k = tid; k < nf; k += TRIM_THREADS) mx = max_keep_nan(mx, m[k]);
    red[tid] = mx;
    if (tid == 0) { first_s = nf; last_s = -1; }
    __syncthreads();
    for (int s = TRIM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = max_keep_nan(red[tid], red[tid + s]);
        __syncthreads();
    }
    // A NaN sample makes its frames' mse and so the maximum NaN: ref is NaN, every comparison below is false and the
    // bounds are (0, 0), as numpy decides; a +-Inf sample ends there too (Inf - Inf in its frames, -Inf in the others).
    const double ref = 10.0 * log10(red[0] != red[0] ? red[0] : fmax(1e-10, red[0]));
    int first = nf, last = -1;
    for (int k = tid; k < nf; k += TRIM_THREADS)
        if (10.0 * log10(fmax(1e-10, m[k])) - ref > -top_db) {
            first = min(first, k);
            last = max(last, k);
        }
    atomicMin(&first_s, first);
    atomicMax(&last_s, last);
    __syncthreads();
    if (tid == 0) {
        long long start = 0, end = 0;   // (no frame qualifies: a non-finite sample; top_db <= 0 is refused by the host)
        if (last_s >= 0) {
            start = (long long)first_s * H;
            const long long e = (long long)(last_s + 1) * H;
            end = e < r.n ? e : (long long)r.n;
        }
        bounds[2 * b] = start;
        bounds[2 * b + 1] = end;
    }
}

// ------------------------------------------------------------------------------------------------ rows of one frame
// mag: the frame's F magnitudes in LDS (visible to the threads that call this); threads `t0, t0 + step, ...` form the bands
__device__ __forceinline__ void feat_mel_row(const FeatArgs& a, const float* mag, long long g, int t0, int step) {
    float* mrow = a.mel_out + g * a.n_mels;
    for (int m = t0; m < a.n_mels; m += step) {
        const int lo = a.mel_band[3 * m], wo = a.mel_band[3 * m + 1], hi = a.mel_band[3 * m + 2];
        float acc = 0.f;
        for (int k = lo; k < hi; ++k) acc = fmaf(a.mel_w[wo + k - lo], mag[k], acc);
        mrow[m] = feat_db(acc, a.norm, a.mel_ref, a.mel_range);
    }
}

// ------------------------------------------------------------------------------------------------ n_fft 2048
// The frame is formed and transformed exactly as stft_kernel (griffin_lim.hip) does for tts_stft, on the segment.
__global__ __launch_bounds__(FEAT_THREADS) void feat2048_kernel(FeatArgs a, const cf* __restrict__ tw1024,
                                                               const cf* __restrict__ tw2048) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int MH = 1024, NF = 2048, F = MH + 1;
    cf* ex_all = reinterpret_cast<cf*>(smem_raw);
    cf* twR = ex_all + FEAT_NW * EX_CPLX;
    cf* twA = twR + 1024;
    float* wtab = reinterpret_cast<float*>(twA + 15 * 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cf* ex = ex_all + wave * EX_CPLX;
    for (int i = tid; i < a.win; i += FEAT_THREADS) wtab[i] = a.window[i];
    for (int i = tid; i < 1024; i += FEAT_THREADS) twR[i] = tw2048[i];
    for (int i = tid; i < 15 * 64; i += FEAT_THREADS) twA[i] = tw1024[(i & 63) * ((i >> 6) + 1)];
    FftTw tw;
#pragma unroll
    for (int d = 1; d < 4; ++d) tw.b[d - 1] = tw1024[16 * (lane & 15) * d];
    tw.a = twA + lane;
    __syncthreads();
    const long long g = (long long)blockIdx.x * FEAT_NW + wave;
    if (g >= a.rows) return;
    const int b = find_item(a.desc, a.B, g, [](const FeatDesc& x) { return x.row0; });
    const FeatDesc r = a.desc[b];
    const int t = (int)(g - r.row0);
    float* lrow = a.lin_out + g * F;
    if (t >= r.Tf) {   // reduction padding
        for (int k = lane; k < F; k += 64) lrow[k] = 0.f;
        for (int m = lane; m < a.n_mels; m += 64) a.mel_out[g * a.n_mels + m] = 0.f;
        return;
    }
    const float* y = a.wav + r.start;
    const int n = r.len;
    const int wpad = (NF - a.win) >> 1;
    const long long ylo = (long long)t * a.hop + wpad - MH;
    cf v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int nn = 2 * (lane + 64 * j);
        float x[2] = {0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int nw = nn + e - wpad;
            if (nw >= 0 && nw < a.win) x[e] = wtab[nw] * y[reflect_index(ylo + nw, n)];
        }
        v[j] = cmk(x[0], x[1]);
    }
    fft1024(v, ex, tw, lane);
#pragma unroll
    for (int c = 0; c < 16; ++c) ex[lane + 64 * c] = v[c];
    wave_lds_sync();
    float mg[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int k = lane + 64 * c;
        const cf zk = v[c];
        const cf zr = ex[(MH - k) & (MH - 1)];
        const cf e = cscale(cadd_conj(zk, zr), 0.5f);
        const cf o = cmul(cscale(csub_conj(zk, zr), 0.5f), twR[k]);
        const cf X = cadd_mi(e, o);
        mg[c] = sqrtf(X.x * X.x + X.y * X.y);
    }
    const float nyq = fabsf(v[0].x - v[0].y);
    wave_lds_sync();
    float* mag = reinterpret_cast<float*>(ex);   // F floats fit in the wave's exchange buffer (2 EX_CPLX)
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int k = lane + 64 * c;
        mag[k] = mg[c];
        lrow[k] = feat_db(mg[c], a.norm, a.lin_ref, a.lin_range);
    }
    if (lane == 0) {
        mag[MH] = nyq;
        lrow[MH] = feat_db(nyq, a.norm, a.lin_ref, a.lin_range);
    }
    wave_lds_sync();
    feat_mel_row(a, mag, g, lane, 64);
}

// ------------------------------------------------------------------------------------------------ any power-of-two n_fft
// The frame and the split / merge pass of glg_stft_kernel (griffin_lim_generic.hip), on the segment.
__global__ __launch_bounds__(FEAT_GTHREADS) void feat_generic_kernel(FeatArgs a, const gcf* __restrict__ tw, int N, int m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = N >> 1, mm = m - 1, H = N >> 1, F = H + 1;
    gcf* z = reinterpret_cast<gcf*>(smem);
    float* mag = reinterpret_cast<float*>(z + M);
    const long long g = blockIdx.x;
    const int b = find_item(a.desc, a.B, g, [](const FeatDesc& x) { return x.row0; });
    const FeatDesc r = a.desc[b];
    const int t = (int)(g - r.row0);
    float* lrow = a.lin_out + g * F;
    if (t >= r.Tf) {
        for (int k = threadIdx.x; k < F; k += blockDim.x) lrow[k] = 0.f;
        for (int q = threadIdx.x; q < a.n_mels; q += blockDim.x) a.mel_out[g * a.n_mels + q] = 0.f;
        return;
    }
    const float* y = a.wav + r.start;
    const int n = r.len, pad = (N - a.win) >> 1;
    const long long y0 = (long long)t * a.hop - H;
    auto sample = [&](int j) -> float {
        const int jw = j - pad;
        if (jw < 0 || jw >= a.win) return 0.f;
        return a.window[jw] * y[reflect_index(y0 + j, n)];
    };
    for (int q = threadIdx.x; q < M; q += blockDim.x) z[glg_bitrev(q, mm)] = (gcf){sample(2 * q), sample(2 * q + 1)};
    glg_fft<false>(z, tw, M, mm);   // (ends with a barrier)
    for (int k = threadIdx.x; k <= H; k += blockDim.x) {
        const gcf zk = z[k & (M - 1)], zm = gconj(z[(M - k) & (M - 1)]);
        gcf X;
        if (k == 0) X = (gcf){zk.x + zk.y, 0.f};
        else if (k == M) X = (gcf){zk.x - zk.y, 0.f};
        else {
            const gcf e = zk + zm, d = gmul(tw[k], zk - zm);
            X = (gcf){0.5f * (e.x + d.y), 0.5f * (e.y - d.x)};
        }
        const float mk = sqrtf(X.x * X.x + X.y * X.y);
        mag[k] = mk;
        lrow[k] = feat_db(mk, a.norm, a.lin_ref, a.lin_range);
    }
    __syncthreads();
    feat_mel_row(a, mag, g, threadIdx.x, blockDim.x);
}

static size_t feat2048_lds(int win) {
    return (size_t)(FEAT_NW * EX_CPLX + 1024 + 15 * 64) * sizeof(cf) + (size_t)((win + 3) & ~3) * sizeof(float);
}

}  // namespace tts

using namespace tts;

// ================================================================================================ host side
namespace {

bool pow2_in(int x, int lo, int hi) { return x >= lo && x <= hi && (x & (x - 1)) == 0; }

// Descriptors go to the device through a pinned buffer of the handle; the previous upload from it must have been read first.
int stage_upload(tts_handle_t h, const void* src, size_t bytes, void* dst) {
    auto& f = h->feat;
    HIPCHK(h, f.staged.sync());
    if (f.staging_bytes < bytes) {
        if (f.staging) HIPCHK(h, hipHostFree(f.staging));
        f.staging = nullptr;
        f.staging_bytes = 0;
        HIPCHK(h, hipHostMalloc(&f.staging, bytes, hipHostMallocDefault));
        f.staging_bytes = bytes;
    }
    std::memcpy(f.staging, src, bytes);
    HIPCHK(h, hipMemcpyAsync(dst, f.staging, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, f.staged.record(h->stream));
    return TTS_OK;
}

int check_offsets(tts_handle_t h, const int64_t* offsets, int B, const char* who) {
    if (!offsets || B < 1 || B > (1 << 24)) return fail(h, TTS_ERR_INVALID, std::string(who) + ": bad offsets / B");
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (offsets[b] < 0 || n < 0 || n >= (int64_t)1 << 31)
            return fail(h, TTS_ERR_INVALID, std::string(who) + ": offsets must be non-negative, non-decreasing and each "
                                                                "recording shorter than 2^31 samples (recording " +
                                                    std::to_string(b) + ")");
    }
    return TTS_OK;
}

int check_params(tts_handle_t h, const tts_feature_params_t* p) {
    if (!p || p->struct_size != (int32_t)sizeof(tts_feature_params_t))
        return fail(h, TTS_ERR_INVALID, "features: params missing or not from tts_default_feature_params (struct_size)");
    if (!pow2_in(p->n_fft, 256, 4096))
        return fail(h, TTS_ERR_UNSUPPORTED, "features: n_fft must be a power of two from 256 to 4096");
    if (p->win_length < 2 || p->win_length > p->n_fft || p->hop_length < 1)
        return fail(h, TTS_ERR_INVALID, "features: need 2 <= win_length <= n_fft, hop_length >= 1");
    if (p->sampling_rate < 1 || p->n_mels < 1 || p->n_mels > 4096 || p->reduction < 1 || !(p->fmin >= 0.f))
        return fail(h, TTS_ERR_INVALID, "features: bad sampling_rate / n_mels / fmin / reduction");
    if (p->trim && (p->trim_frame_length < 2 || p->trim_hop_length < 1 || !(p->trim_top_db > 0.f)))
        return fail(h, TTS_ERR_INVALID, "features: trim needs frame_length >= 2, hop_length >= 1, top_db > 0");
    return TTS_OK;
}

int trim_enqueue(tts_handle_t h, const float* wav, const int64_t* offsets, int B, int L, int H, float top_db,
                 int64_t* bounds) {
    std::vector<TrimDesc> d(B);
    long long items = 0;
    for (int b = 0; b < B; ++b) {
        const int n = (int)(offsets[b + 1] - offsets[b]);
        if (n <= L / 2)
            return fail(h, TTS_ERR_INVALID, "trim: recording " + std::to_string(b) + " has " + std::to_string(n) +
                                                " samples, at most frame_length / 2 (reflect padding undefined)");
        d[b] = TrimDesc{offsets[b], items, n, 0};
        items += n / H + 1;
    }
    WS(h, "feat.trim_desc", TrimDesc, B, dd);
    WS(h, "feat.mse", double, items, mse);
    int rc = stage_upload(h, d.data(), sizeof(TrimDesc) * B, dd);
    if (rc) return rc;
    ProfScope ps(h, ST_FEATURES, 2);
    const long long blocks = (items + TRIM_THREADS / 64 - 1) / (TRIM_THREADS / 64);
    hipLaunchKernelGGL(trim_mse_kernel, dim3((unsigned)blocks), dim3(TRIM_THREADS), 0, h->stream, wav, dd, B, items, L, H, mse);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(TRIM_THREADS), 0, h->stream, dd, mse, H, (double)top_db,
                       reinterpret_cast<long long*>(bounds));
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}

// window and compact HTK mel filterbank of the configuration (librosa.filters.mel(htk=True, norm=1) [librosa-0.6], as
// tts_mel_spectrogram builds it), cached on the handle
int feat_tables(tts_handle_t h, const tts_feature_params_t* p) {
    auto& f = h->feat;
    const float fmax = p->fmax > 0 ? p->fmax : p->sampling_rate / 2.0f;
    const bool win_ok = f.window && f.win == p->win_length;
    const bool mel_ok = f.mel_w && f.n_fft == p->n_fft && f.sr == p->sampling_rate && f.n_mels == p->n_mels &&
                        f.fmin == p->fmin && f.fmax == fmax;
    if (win_ok && mel_ok) return TTS_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (a configuration change: the tables may still be in use)
    if (!win_ok) {
        if (f.window) HIPCHK(h, hipFree(f.window));
        f.window = nullptr;
        std::vector<float> w(p->win_length);
        for (int i = 0; i < p->win_length; ++i) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / p->win_length));
        HIPCHK(h, hipMalloc(&f.window, w.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(f.window, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        f.win = p->win_length;
    }
    if (!mel_ok) {
        if (f.mel_w) HIPCHK(h, hipFree(f.mel_w));
        if (f.mel_band) HIPCHK(h, hipFree(f.mel_band));
        f.mel_w = nullptr;
        f.mel_band = nullptr;
        const int F = 1 + p->n_fft / 2, nm = p->n_mels, sr = p->sampling_rate;
        auto hz2mel = [](double x) { return 2595.0 * std::log10(1.0 + x / 700.0); };
        auto mel2hz = [](double x) { return 700.0 * (std::pow(10.0, x / 2595.0) - 1.0); };
        std::vector<double> mel_f(nm + 2);
        const double m0 = hz2mel(p->fmin), m1 = hz2mel(fmax);
        for (int i = 0; i < nm + 2; ++i) mel_f[i] = mel2hz(m0 + (m1 - m0) * i / (nm + 1));
        std::vector<float> w;
        std::vector<int> band(3 * nm);
        std::vector<float> row(F);
        for (int i = 0; i < nm; ++i) {
            const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
            int lo = F, hi = 0;
            for (int k = 0; k < F; ++k) {
                const double freq = (sr / 2.0) * k / (F - 1);
                const double lower = (freq - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
                const double upper = (mel_f[i + 2] - freq) / (mel_f[i + 2] - mel_f[i + 1]);
                row[k] = (float)(std::max(0.0, std::min(lower, upper)) * enorm);
                if (row[k] != 0.f) { lo = std::min(lo, k); hi = k + 1; }
            }
            if (hi <= lo) lo = hi = 0;
            band[3 * i] = lo;
            band[3 * i + 1] = (int)w.size();
            band[3 * i + 2] = hi;
            for (int k = lo; k < hi; ++k) w.push_back(row[k]);
        }
        if (w.empty()) w.push_back(0.f);
        HIPCHK(h, hipMalloc(&f.mel_w, w.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(f.mel_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMalloc(&f.mel_band, band.size() * sizeof(int)));
        HIPCHK(h, hipMemcpy(f.mel_band, band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice));
        f.n_fft = p->n_fft; f.sr = sr; f.n_mels = nm; f.fmin = p->fmin; f.fmax = fmax;
    }
    return TTS_OK;
}

}  // namespace

namespace tts_api {
void feat_release(tts_handle_t h) {
    auto& f = h->feat;
    if (f.window) hipFree(f.window);
    if (f.mel_w) hipFree(f.mel_w);
    if (f.mel_band) hipFree(f.mel_band);
    f.staged.sync();   // (tts_destroy only, in front of `delete h`: the pointers are not used again, the event goes with the handle)
    if (f.staging) hipHostFree(f.staging);
}
}  // namespace tts_api

int tts_default_feature_params(tts_feature_params_t* p) {
    if (!p) return TTS_ERR_INVALID;
    *p = tts_feature_params_t{};
    p->struct_size = (int32_t)sizeof(tts_feature_params_t);
    p->n_fft = 2048;
    p->win_length = 1102;
    p->hop_length = 275;
    p->sampling_rate = 22050;
    p->n_mels = 80;
    p->fmin = 0.f;
    p->fmax = 8000.f;
    p->mel_ref_db = 6.02f;
    p->mel_max_db = 99.89f;
    p->linear_ref_db = 35.66f;
    p->linear_max_db = 100.f;
    p->normalize = 1;
    p->reduction = 5;
    p->trim = 1;
    p->trim_top_db = 60.f;
    p->trim_frame_length = 2048;
    p->trim_hop_length = 512;
    return TTS_OK;
}

int tts_trim_bounds(tts_handle_t h, const float* wav, const int64_t* offsets, int B, int frame_length, int hop_length,
                    float top_db, int64_t* bounds) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    if (!wav || !bounds || frame_length < 2 || hop_length < 1 || !(top_db > 0.f))
        return fail(h, TTS_ERR_INVALID, "trim_bounds: bad arguments (frame_length >= 2, hop_length >= 1, top_db > 0)");
    int rc = check_offsets(h, offsets, B, "trim_bounds");
    if (rc) return rc;
    return trim_enqueue(h, wav, offsets, B, frame_length, hop_length, top_db, bounds);
}

int tts_plan_features(tts_handle_t h, const float* wav, const int64_t* offsets, int B, const tts_feature_params_t* p,
                      int64_t* plan) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    if (!wav || !plan) return fail(h, TTS_ERR_INVALID, "plan_features: bad arguments");
    int rc = check_params(h, p);
    if (rc) return rc;
    if ((rc = check_offsets(h, offsets, B, "plan_features"))) return rc;
    std::vector<int64_t> bounds(2 * (size_t)B);
    if (p->trim) {
        WS(h, "feat.bounds", int64_t, 2 * (size_t)B, db);
        if ((rc = trim_enqueue(h, wav, offsets, B, p->trim_frame_length, p->trim_hop_length, p->trim_top_db, db))) return rc;
        HIPCHK(h, hipMemcpyAsync(bounds.data(), db, bounds.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));   // the one device -> host synchronisation of a batch
    } else {
        for (int b = 0; b < B; ++b) {
            bounds[2 * b] = 0;
            bounds[2 * b + 1] = offsets[b + 1] - offsets[b];
        }
    }
    for (int b = 0; b < B; ++b) {
        const int64_t len = bounds[2 * b + 1] - bounds[2 * b];
        if (len <= p->n_fft / 2)
            return fail(h, TTS_ERR_INVALID, "plan_features: recording " + std::to_string(b) + ": the analysed segment has " +
                                                std::to_string(len) + " samples, at most n_fft / 2 (reflect padding undefined)");
        const int64_t Tf = 1 + len / p->hop_length;
        plan[3 * b] = bounds[2 * b];
        plan[3 * b + 1] = bounds[2 * b + 1];
        plan[3 * b + 2] = (Tf + p->reduction - 1) / p->reduction * p->reduction;
    }
    return TTS_OK;
}

int tts_extract_features(tts_handle_t h, const float* wav, const int64_t* offsets, int B, const tts_feature_params_t* p,
                         const int64_t* plan, float* mel_out, float* lin_out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    if (!wav || !plan || !mel_out || !lin_out) return fail(h, TTS_ERR_INVALID, "extract_features: bad arguments");
    if (((uintptr_t)mel_out | (uintptr_t)lin_out | (uintptr_t)wav) & 3)
        return fail(h, TTS_ERR_INVALID, "extract_features: float buffers must be 4-byte aligned");
    int rc = check_params(h, p);
    if (rc) return rc;
    if ((rc = check_offsets(h, offsets, B, "extract_features"))) return rc;
    std::vector<FeatDesc> d(B);
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b], s = plan[3 * b], e = plan[3 * b + 1], tp = plan[3 * b + 2];
        const int64_t Tf = 1 + (e - s) / p->hop_length;
        if (s < 0 || e > n || e - s <= p->n_fft / 2 || tp != (Tf + p->reduction - 1) / p->reduction * p->reduction)
            return fail(h, TTS_ERR_INVALID, "extract_features: plan entry " + std::to_string(b) +
                                                " does not match the recording and parameters (from tts_plan_features)");
        d[b] = FeatDesc{offsets[b] + s, rows, (int)(e - s), (int)Tf};
        rows += tp;
    }
    if (rows >= (1ll << 31)) return fail(h, TTS_ERR_INVALID, "extract_features: too many frames");
    if ((rc = feat_tables(h, p))) return rc;
    const bool fast = p->n_fft == TTS_GL_NFFT;
    const float2* tw = nullptr;
    if (fast) {
        if ((rc = gl_tables(h))) return rc;
    } else if ((rc = glg_twiddles(h, p->n_fft, &tw))) {
        return rc;
    }
    WS(h, "feat.desc", FeatDesc, B, dd);
    if ((rc = stage_upload(h, d.data(), sizeof(FeatDesc) * B, dd))) return rc;
    FeatArgs a{};
    a.wav = wav;
    a.desc = dd;
    a.B = B;
    a.rows = rows;
    a.window = h->feat.window;
    a.win = p->win_length;
    a.hop = p->hop_length;
    a.n_mels = p->n_mels;
    a.mel_w = h->feat.mel_w;
    a.mel_band = h->feat.mel_band;
    a.norm = p->normalize ? 1 : 0;
    a.mel_ref = p->mel_ref_db;
    a.mel_range = fabsf(p->mel_ref_db) + fabsf(p->mel_max_db);
    a.lin_ref = p->linear_ref_db;
    a.lin_range = fabsf(p->linear_ref_db) + fabsf(p->linear_max_db);
    a.mel_out = mel_out;
    a.lin_out = lin_out;
    ProfScope ps(h, ST_FEATURES, 1);
    if (fast) {
        const size_t lds = feat2048_lds(p->win_length);
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&feat2048_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(feat2048_kernel, dim3((unsigned)((rows + FEAT_NW - 1) / FEAT_NW)), dim3(FEAT_THREADS), lds,
                           h->stream, a, reinterpret_cast<const cf*>(h->gl.tw1024), reinterpret_cast<const cf*>(h->gl.tw2048));
    } else {
        int m = 0;
        while ((1 << m) < p->n_fft) ++m;
        const size_t lds = (size_t)(p->n_fft / 2) * sizeof(gcf) + (size_t)(p->n_fft / 2 + 1) * sizeof(float);
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&feat_generic_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(feat_generic_kernel, dim3((unsigned)rows), dim3(FEAT_GTHREADS), lds, h->stream, a,
                           reinterpret_cast<const gcf*>(tw), p->n_fft, m);
    }
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}
