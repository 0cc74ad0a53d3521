// Mel-frequency cepstral coefficients of time-major mel rows: the DCT of calculate_mfccs.
//   calculate_mfccs             reference audio/features.py:89-113: librosa.feature.mfcc(S=mel_spec, n_mfcc=n) = the orthonormal
//                               DCT-II of S along the mel axis, first n rows (no dB conversion of its own)
//   out[b][t][k] = (float) sum_n d[k][n] x[n], x[n] = (double)spec[b][t][n] or np.clip(spec, 0, 1) of it, in double, n ascending,
//   rounded once; rows t >= n_frames[b] are never read and written as 0.
// A workgroup stages MFCC_ROWS frames in LDS (clipped, as float: the conversion to double is exact) and its threads take one
// (frame, coefficient) each; the table d is laid out [n][k], so a wave's loads of it are contiguous.  No atomics; a frame's
// coefficients depend on that frame alone.  The lengths travel by value in the kernel arguments, MFCC_UTTS utterances per launch.
#include "api_internal.h"
#include "cepstrum_plan.h"

namespace tts {

constexpr int MFCC_THREADS = 256;
constexpr int MFCC_ROWS = 8;   // frames a workgroup stages per round: 8 x 1024 floats = 32 KiB at the largest n_mels

struct MfccLens {
    int n[MFCC_UTTS];
};

// np.clip(x, 0, 1): a NaN fails both comparisons and stays
__device__ __forceinline__ float mfcc_clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

__global__ __launch_bounds__(MFCC_THREADS) void mfcc_kernel(const float* __restrict__ spec, float* __restrict__ out, const double* __restrict__ tab,
                                                            MfccLens lens, int nb, int T, int n_mels, int stride, int n_mfcc, int clip01) {
    __shared__ float xs[MFCC_ROWS * MFCC_MAX_MELS];
    const long long rows = (long long)nb * T;
    for (long long r0 = (long long)blockIdx.x * MFCC_ROWS; r0 < rows; r0 += (long long)gridDim.x * MFCC_ROWS) {   // (uniform)
        const int nr = (int)min((long long)MFCC_ROWS, rows - r0);
        for (int e = threadIdx.x; e < nr * n_mels; e += MFCC_THREADS) {
            const int r = e / n_mels, n = e - r * n_mels;
            const long long row = r0 + r;
            const int b = (int)(row / T), t = (int)(row - (long long)b * T);
            float x = 0.f;
            if (t < lens.n[b]) {
                x = spec[(size_t)row * stride + n];
                if (clip01) x = mfcc_clip01(x);
            }
            xs[r * n_mels + n] = x;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nr * n_mfcc; e += MFCC_THREADS) {
            const int r = e / n_mfcc, k = e - r * n_mfcc;
            const long long row = r0 + r;
            const int b = (int)(row / T), t = (int)(row - (long long)b * T);
            float y = 0.f;
            if (t < lens.n[b]) {
                const float* x = xs + r * n_mels;
                double acc = 0.0;
                for (int n = 0; n < n_mels; ++n) acc += tab[(size_t)n * n_mfcc + k] * (double)x[n];
                y = (float)acc;
            }
            out[(size_t)row * n_mfcc + k] = y;
        }
        __syncthreads();
    }
}

}  // namespace tts

namespace tts_api {

// the table of (n_mels, n_mfcc) on the device: built on the host in double at the first call that asks for it, uploaded with a
// synchronous copy and kept by the handle
static int mfcc_table_dev(tts_handle_t h, int n_mels, int n_mfcc, const double** out) {
    const uint64_t key = ((uint64_t)n_mels << 32) | (uint64_t)n_mfcc;
    auto it = h->mfcc_tabs.find(key);
    if (it == h->mfcc_tabs.end()) {
        const std::vector<double> host = mfcc_table(n_mels, n_mfcc);
        double* dev = nullptr;
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&dev), host.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(dev);
            HIPCHK(h, e);
        }
        it = h->mfcc_tabs.emplace(key, dev).first;
    }
    *out = it->second;
    return TTS_OK;
}

void mfcc_release(tts_handle_t h) {
    for (auto& kv : h->mfcc_tabs) hipFree(kv.second);
    h->mfcc_tabs.clear();
}

}  // namespace tts_api

extern "C" {

int tts_mfcc(tts_handle_t h, const float* spec, int B, int T, int n_mels, int row_stride, const int32_t* n_frames, int n_mfcc, int clip01,
             float* out) {
    DeviceScope dev_scope(h);
    const std::string why = mfcc_check(spec && out, B, T, n_mels, row_stride, n_frames, n_mfcc);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "mfcc: " + why);
    if (!h) return TTS_ERR_INVALID;
    const double* tab = nullptr;
    int rc = mfcc_table_dev(h, n_mels, n_mfcc, &tab);
    if (rc) return rc;
    ProfScope ps(h, ST_MFCC, length_chunks(B, MFCC_UTTS));
    for (int b0 = 0; b0 < B; b0 += MFCC_UTTS) {
        const int nb = std::min(MFCC_UTTS, B - b0);
        MfccLens lens;
        fill_lengths(lens.n, n_frames, b0, nb, T);
        const long long want = ((long long)nb * T + MFCC_ROWS - 1) / MFCC_ROWS;
        const unsigned grid = (unsigned)std::min<long long>(want, 1 << 16);   // (the rows beyond take another round)
        hipLaunchKernelGGL(mfcc_kernel, dim3(grid), dim3(MFCC_THREADS), 0, h->stream, spec + (size_t)b0 * T * row_stride,
                           out + (size_t)b0 * T * n_mfcc, tab, lens, nb, T, n_mels, row_stride, n_mfcc, clip01 != 0 ? 1 : 0);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // extern "C"
