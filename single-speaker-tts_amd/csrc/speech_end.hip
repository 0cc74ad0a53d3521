// End of speech: which frames of a spectrogram are above a threshold, and the frame count that follows from the last of them.
//   silence_interval_from_spectrogram    reference audio/effects.py:218-233 (np.max over the bins of a frame > threshold_db,
//                                        trim_end = the last such frame) -- the criterion of the TODO at tacotron/inference.py:76-78
// A streaming reduction: every float of the batch is read once (262 MB at 64 x 1000 x 1025), nothing is computed on the data --
// maxima and one comparison -- so the result is exact.  Two launches: the rows (one wave each), then the utterances.
// tts_speech_interval is the whole of the reference's function, (trim_start, trim_end): the same rows, then both ends.
#include "api_internal.h"

namespace tts {

constexpr int SE_THREADS = 256;
constexpr int SE_ROWS = SE_THREADS / 64;   // rows a workgroup takes per round, one per wave

// active[row] = np.max(spec[row][0 .. F)) > thr as numpy evaluates it: a NaN anywhere in the row makes np.max NaN and the
// comparison False.  fmaxf drops a NaN operand, so the NaNs are counted beside the maximum instead of travelling in it.
// Columns F .. stride - 1 are never read.  A row is read in 16-byte loads from its first 16-byte boundary on (rows of 1025
// floats start at every alignment), the up to three floats in front of it and behind the last whole load one by one.
__global__ __launch_bounds__(SE_THREADS) void speech_rows_kernel(const float* __restrict__ spec, long long rows, int F, int stride, float thr,
                                                                 unsigned char* __restrict__ active) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * SE_ROWS + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * SE_ROWS) {   // (wave-uniform)
        const float* p = spec + (size_t)row * stride;
        int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
        head = head < F ? head : F;
        const int nvec = (F - head) >> 2;
        float mx = -INFINITY;
        bool nan = false;
        if (lane < head) {
            const float v = p[lane];
            nan |= v != v;
            mx = fmaxf(mx, v);
        }
        const float4* pv = reinterpret_cast<const float4*>(p + head);
        for (int i = lane; i < nvec; i += 64) {
            const float4 v = pv[i];
            nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
            mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
        }
        const int tail = head + 4 * nvec + lane;   // (at most three floats are left)
        if (tail < F) {
            const float v = p[tail];
            nan |= v != v;
            mx = fmaxf(mx, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const bool any_nan = __ballot(nan) != 0;
        if (lane == 0) active[row] = (!any_nan && mx > thr) ? 1 : 0;
    }
}

// last_active[b] = the largest t with active[b][t], -1 without one; n_frames[b] = min(T, max(min_frames, last + 1 + keep))
__global__ __launch_bounds__(SE_THREADS) void speech_last_kernel(const unsigned char* __restrict__ active, int T, int keep, int min_frames,
                                                                 int* __restrict__ n_frames, int* __restrict__ last_active) {
    __shared__ int red[SE_THREADS / 64];
    const int b = blockIdx.x;
    const unsigned char* a = active + (size_t)b * T;
    int last = -1;
    for (int t = threadIdx.x; t < T; t += SE_THREADS)
        if (a[t]) last = t;   // (ascending: the thread's largest)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SE_THREADS / 64; ++w) last = max(last, red[w]);
        if (last_active) last_active[b] = last;
        long long n = (long long)last + 1 + keep;
        n = n < min_frames ? min_frames : n;
        n_frames[b] = (int)(n > T ? T : n);
    }
}

// first_active[b] = the smallest t with active[b][t], last_active[b] = the largest; both -1 without one
__global__ __launch_bounds__(SE_THREADS) void speech_interval_kernel(const unsigned char* __restrict__ active, int T, int* __restrict__ first_active,
                                                                     int* __restrict__ last_active) {
    __shared__ int red[2][SE_THREADS / 64];
    const int b = blockIdx.x;
    const unsigned char* a = active + (size_t)b * T;
    int first = T, last = -1;   // (T: none so far)
    for (int t = threadIdx.x; t < T; t += SE_THREADS)
        if (a[t]) {
            first = min(first, t);
            last = t;   // (ascending: the thread's largest)
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        first = min(first, __shfl_xor(first, o));
        last = max(last, __shfl_xor(last, o));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = first;
        red[1][threadIdx.x >> 6] = last;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SE_THREADS / 64; ++w) {
            first = min(first, red[0][w]);
            last = max(last, red[1][w]);
        }
        first_active[b] = last < 0 ? -1 : first;
        last_active[b] = last;
    }
}

}  // namespace tts

namespace tts_api {

int speech_threshold(float threshold_db, float ref_db, float max_db, float power, int units, float* out) {
    if (!out || threshold_db != threshold_db) return TTS_ERR_INVALID;
    double v;
    if (units == TTS_SPEECH_NORMALIZED_DB) {
        const double range = std::fabs((double)ref_db) + std::fabs((double)max_db);
        if (ref_db != ref_db || max_db != max_db || !(range > 0.0)) return TTS_ERR_INVALID;
        v = ((double)threshold_db - (double)ref_db) / range + 1.0;
    } else if (units == TTS_SPEECH_MAGNITUDE_POWER) {
        if (!(power > 0.f)) return TTS_ERR_INVALID;
        v = std::pow(std::pow(10.0, (double)threshold_db / 20.0), (double)power);
    } else {
        return TTS_ERR_INVALID;
    }
    *out = (float)v;
    return TTS_OK;
}

// The detection's row flags for B utterances of T frames; with_frames: and the lengths of a synthesis call on the device.
int eos_scratch(tts_handle_t h, int B, int T, bool with_frames, EosScratch* s) {
    WS(h, "eos.active", unsigned char, (size_t)B * T, active);
    *s = EosScratch{active, nullptr};
    if (with_frames) {
        WS(h, "eos.frames", int32_t, (size_t)B, frames);
        s->frames = frames;
    }
    return TTS_OK;
}

int speech_frames_impl(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold, int keep_frames,
                       int min_frames, int32_t* n_frames, int32_t* last_active) {
    if (!spec || !n_frames) return fail(h, TTS_ERR_INVALID, "speech_frames: spec and n_frames must not be NULL");
    if (B < 1 || T < 1 || F < 1) return fail(h, TTS_ERR_INVALID, "speech_frames: need B, T, F >= 1");
    if (row_stride < F) return fail(h, TTS_ERR_INVALID, "speech_frames: row_stride < F");
    if (keep_frames < 0) return fail(h, TTS_ERR_INVALID, "speech_frames: keep_frames < 0");
    if (min_frames < 1 || min_frames > T) return fail(h, TTS_ERR_INVALID, "speech_frames: min_frames must lie in [1, T]");
    if (threshold != threshold) return fail(h, TTS_ERR_INVALID, "speech_frames: the threshold is NaN");
    const long long rows = (long long)B * T;
    EosScratch s;
    const int rc = eos_scratch(h, B, T, false, &s);
    if (rc) return rc;
    ProfScope ps(h, ST_SPEECH_END, 2);
    const long long want = (rows + SE_ROWS - 1) / SE_ROWS;
    const unsigned grid = (unsigned)std::min<long long>(want, 1 << 18);   // (the rows beyond take another round)
    hipLaunchKernelGGL(speech_rows_kernel, dim3(grid), dim3(SE_THREADS), 0, h->stream, spec, rows, F, row_stride, threshold, s.active);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(speech_last_kernel, dim3((unsigned)B), dim3(SE_THREADS), 0, h->stream, s.active, T, keep_frames, min_frames,
                       n_frames, last_active);
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}

int speech_interval_impl(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold, int32_t* first_active,
                         int32_t* last_active) {
    if (!spec || !first_active || !last_active) return fail(h, TTS_ERR_INVALID, "speech_interval: spec, first_active and last_active must not be NULL");
    if (B < 1 || T < 1 || F < 1) return fail(h, TTS_ERR_INVALID, "speech_interval: need B, T, F >= 1");
    if (row_stride < F) return fail(h, TTS_ERR_INVALID, "speech_interval: row_stride < F");
    if (threshold != threshold) return fail(h, TTS_ERR_INVALID, "speech_interval: the threshold is NaN");
    if (!h) return TTS_ERR_INVALID;
    const long long rows = (long long)B * T;
    WS(h, "eos.interval_active", unsigned char, (size_t)rows, active);   // (its own: nothing orders it behind a synthesis call's eos.active)
    ProfScope ps(h, ST_SPEECH_END, 2);
    const long long want = (rows + SE_ROWS - 1) / SE_ROWS;
    const unsigned grid = (unsigned)std::min<long long>(want, 1 << 18);   // (the rows beyond take another round)
    hipLaunchKernelGGL(speech_rows_kernel, dim3(grid), dim3(SE_THREADS), 0, h->stream, spec, rows, F, row_stride, threshold, active);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(speech_interval_kernel, dim3((unsigned)B), dim3(SE_THREADS), 0, h->stream, active, T, first_active, last_active);
    HIPCHK(h, hipGetLastError());
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_speech_frames(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold, int keep_frames,
                      int min_frames, int32_t* n_frames, int32_t* last_active) {
    DeviceScope dev_scope(h);
    if (!h) return TTS_ERR_INVALID;
    return speech_frames_impl(h, spec, B, T, F, row_stride, threshold, keep_frames, min_frames, n_frames, last_active);
}

int tts_speech_interval(tts_handle_t h, const float* spec, int B, int T, int F, int row_stride, float threshold, int32_t* first_active,
                        int32_t* last_active) {
    DeviceScope dev_scope(h);
    return speech_interval_impl(h, spec, B, T, F, row_stride, threshold, first_active, last_active);
}

int tts_speech_threshold(float threshold_db, float ref_db, float max_db, float power, int units, float* out) {
    return speech_threshold(threshold_db, ref_db, max_db, power, units, out);
}

}  // extern "C"
