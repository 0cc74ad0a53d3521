// Speaking rate: time-stretch of magnitude spectrograms ahead of Griffin-Lim.
//   time_stretch                reference audio/effects.py:46-88: librosa 0.6 phase_vocoder(stft, rate), then np.abs of the result
// The vocoder's phase advance does not survive the np.abs (|mag exp(1j phase)| = mag), so what the reference hands to Griffin-Lim
// is a linear blend of neighbouring magnitude frames at the times k rate:
//   n_out = ceil(n / rate);   s = k rate, i = (int)s, a = s - floor(s);   y[k] = (float)((1 - a) x[i] + a x[i + 1])
// in double, every operation rounded on its own (no FMA), one rounding to float32; columns i >= n are the vocoder's zero padding:
// they read as 0.0 and are never fetched.  The blend is always evaluated: 0 * NaN and 0 * Inf stay NaN, as in numpy.
// One HBM-bound pass, at most two input rows per output row.  Two layouts of the same arithmetic (the same bits): time-major
// padded rows, which the call pipeline holds, and the reference's (F, T).  No atomics; an utterance's output does not depend on
// the batch it is in.  The lengths travel by value in the kernel arguments, ST_CHUNK utterances per launch: nothing is uploaded
// and nothing synchronised.
#include "api_internal.h"
#include "stretch_plan.h"

// No contraction anywhere in this file: (1 - a) x0 + a x1 is two products and a sum, and a = s - floor(s) is a difference of the
// ROUNDED product s = k rate.  The compiler fuses through __dmul_rn / __dadd_rn too, so the file is also built with
// -ffp-contract=off (build.py).
#pragma clang fp contract(off)

namespace tts {

constexpr int ST_THREADS = 256;
constexpr int ST_ROWS = ST_THREADS / 64;   // time-major: output rows a workgroup takes per round, one per wave
constexpr int ST_CHUNK = 64;               // utterances per launch

struct StretchLens {
    int n_in[ST_CHUNK];    // frames of the utterance that may be read
    int n_out[ST_CHUNK];   // stretched_frames(n_in, rate): the frames that are blended; the rest of the row is 0
};

__device__ __forceinline__ float stretch_blend(double w0, double a, float x0, float x1) {
    return (float)__dadd_rn(__dmul_rn(w0, (double)x0), __dmul_rn(a, (double)x1));
}

// in [nb][T][stride] -> out [nb][T_out][stride]; the first F floats of a row are its data, the rest is neither read nor written.
// i and a are computed once per output row, uniform across the wave that takes it.  VEC: stride % 4 == 0 and both buffers are
// 16-byte aligned, so every row is; the rows then move in 16-byte accesses and the up to three floats behind them one by one.
template <bool VEC>
__global__ __launch_bounds__(ST_THREADS) void stretch_rows_kernel(const float* __restrict__ in, float* __restrict__ out, StretchLens lens, int nb,
                                                                  int T, int T_out, int F, int stride, double rate) {
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)nb * T_out;
    for (long long row = (long long)blockIdx.x * ST_ROWS + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * ST_ROWS) {   // (wave-uniform)
        const int b = (int)(row / T_out), k = (int)(row - (long long)b * T_out);
        const int n = lens.n_in[b];
        float* q = out + (size_t)row * stride;
        const double s = __dmul_rn((double)k, rate);
        const int i = (int)s;
        const double a = __dsub_rn(s, floor(s)), w0 = __dsub_rn(1.0, a);
        const bool live = k < lens.n_out[b];
        const bool h0 = live && i < n, h1 = live && i + 1 < n;   // (beyond: the zero padding, never fetched)
        const float* p0 = in + ((size_t)b * T + (h0 ? i : 0)) * stride;
        const float* p1 = in + ((size_t)b * T + (h1 ? i + 1 : 0)) * stride;
        int done = 0;
        if (VEC) {
            const int nvec = F >> 2;
            const float4* v0 = reinterpret_cast<const float4*>(p0);
            const float4* v1 = reinterpret_cast<const float4*>(p1);
            float4* vq = reinterpret_cast<float4*>(q);
            for (int j = lane; j < nvec; j += 64) {
                float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) {
                    const float4 x0 = h0 ? v0[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 x1 = h1 ? v1[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                    y.x = stretch_blend(w0, a, x0.x, x1.x);
                    y.y = stretch_blend(w0, a, x0.y, x1.y);
                    y.z = stretch_blend(w0, a, x0.z, x1.z);
                    y.w = stretch_blend(w0, a, x0.w, x1.w);
                }
                vq[j] = y;
            }
            done = nvec << 2;
        }
        for (int f = done + lane; f < F; f += 64) {
            float y = 0.f;
            if (live) y = stretch_blend(w0, a, h0 ? p0[f] : 0.f, h1 ? p1[f] : 0.f);
            q[f] = y;
        }
    }
}

// in [nb][F][T] -> out [nb][F][T_out], the reference layout: a workgroup per (utterance, bin) row, threads along the output
// frames.  The writes are contiguous; the reads gather along the contiguous axis at stride `rate` (0.25 .. 4 floats), two
// neighbours per output, so a wave's loads fall into the few cache lines its outputs span: no staging.
__global__ __launch_bounds__(ST_THREADS) void stretch_cols_kernel(const float* __restrict__ in, float* __restrict__ out, StretchLens lens, int nb,
                                                                  int F, int T, int T_out, double rate) {
    const long long rows = (long long)nb * F;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int b = (int)(row / F);
        const int n = lens.n_in[b], n_out = lens.n_out[b];
        const float* p = in + (size_t)row * T;
        float* q = out + (size_t)row * T_out;
        for (int k = threadIdx.x; k < T_out; k += ST_THREADS) {
            float y = 0.f;
            if (k < n_out) {
                const double s = __dmul_rn((double)k, rate);
                const int i = (int)s;
                const double a = __dsub_rn(s, floor(s)), w0 = __dsub_rn(1.0, a);
                const float x0 = i < n ? p[i] : 0.f;
                const float x1 = i + 1 < n ? p[i + 1] : 0.f;
                y = stretch_blend(w0, a, x0, x1);
            }
            q[k] = y;
        }
    }
}

}  // namespace tts

namespace tts_api {

// Both layouts (time_major: rows of `row_stride` floats; otherwise the reference's (F, T) and row_stride is ignored), on
// h->stream.  n_frames: HOST lengths or null (all T); they and everything else have been checked (stretch_check).
int stretch_impl(tts_handle_t h, const float* in, int B, int T, int F, int row_stride, bool time_major, const int32_t* n_frames, double rate,
                 int T_out, float* out) {
    ProfScope ps(h, ST_STRETCH, length_chunks(B, ST_CHUNK));
    const size_t per_in = time_major ? (size_t)T * row_stride : (size_t)F * T;
    const size_t per_out = time_major ? (size_t)T_out * row_stride : (size_t)F * T_out;
    const bool vec = time_major && row_stride % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    for (int b0 = 0; b0 < B; b0 += ST_CHUNK) {
        const int nb = std::min(ST_CHUNK, B - b0);
        StretchLens lens = {};
        fill_lengths(lens.n_in, n_frames, b0, nb, T);
        for (int b = 0; b < nb; ++b) lens.n_out[b] = (int)std::min<long long>(stretched_frames(lens.n_in[b], rate), T_out);
        const float* src = in + (size_t)b0 * per_in;
        float* dst = out + (size_t)b0 * per_out;
        if (time_major) {
            const long long want = ((long long)nb * T_out + ST_ROWS - 1) / ST_ROWS;
            const unsigned grid = (unsigned)std::min<long long>(want, 1 << 18);   // (the rows beyond take another round)
            if (vec) hipLaunchKernelGGL(stretch_rows_kernel<true>, dim3(grid), dim3(ST_THREADS), 0, h->stream, src, dst, lens, nb, T, T_out, F, row_stride, rate);
            else hipLaunchKernelGGL(stretch_rows_kernel<false>, dim3(grid), dim3(ST_THREADS), 0, h->stream, src, dst, lens, nb, T, T_out, F, row_stride, rate);
        } else {
            const unsigned grid = (unsigned)std::min<long long>((long long)nb * F, 1 << 20);
            hipLaunchKernelGGL(stretch_cols_kernel, dim3(grid), dim3(ST_THREADS), 0, h->stream, src, dst, lens, nb, F, T, T_out, rate);
        }
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_stretched_frames(int n_frames, double rate, int* out) {
    if (!out || n_frames < 1 || !stretch_rate_ok(rate)) return TTS_ERR_INVALID;
    *out = (int)stretched_frames(n_frames, rate);
    return TTS_OK;
}

int tts_stretch_magnitudes(tts_handle_t h, const float* mag, int B, int F, int T, const int32_t* n_frames, double rate, int T_out, float* out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const std::string why = stretch_check(mag && out, B, F, T, F, n_frames, rate, T_out);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "stretch_magnitudes: " + why);
    return stretch_impl(h, mag, B, T, F, F, false, n_frames, rate, T_out, out);
}

int tts_stretch_rows(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, const int32_t* n_frames, double rate, int T_out,
                     float* out) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    const std::string why = stretch_check(spec && out, B, F, T, row_stride, n_frames, rate, T_out);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "stretch_rows: " + why);
    return stretch_impl(h, spec, B, T, F, row_stride, true, n_frames, rate, T_out, out);
}

}  // extern "C"
