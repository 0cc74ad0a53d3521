// Evaluation losses of Tacotron in Mode.EVAL (reference tacotron/model.py:432-442):
//   loss_decoder         = mean |mel_target - mel_out|   over all B*T*n_mels elements (zero-padded frames included)
//   loss_post_processing = mean |lin_target - lin_out|   over all B*T*F elements
//   loss                 = loss_decoder + loss_post_processing (float32, as TensorFlow forms it)
//
// Two launches, no float atomics, and a summation order fixed by the shapes and the target's address alone:
//   pass 1: each utterance's slab of a tensor (T*C contiguous floats) is cut into chunks of EL_CHUNK floats counted from the
//           16-byte boundary at or before the slab's start (C is odd for F = 1025 / 513 / 129 ..., so slabs start anywhere
//           modulo 16 bytes: the partial quads at the head and the tail are read element by element).  One workgroup reduces
//           one chunk at a time in float64 -- |t - o| in float32 (the elementwise op TF runs), each term widened and added in
//           a fixed per-thread order, then a fixed wave64 xor tree and the four waves in index order -- and stores the chunk's
//           partial.  The workgroups stride over the chunks; WHICH workgroup reduces a chunk never changes its sum, so the
//           bits do not depend on the grid size.
//   pass 2: one workgroup adds each utterance's chunk partials (lane-strided in index order, then the same xor tree) into
//           S[u][0] (mel) / S[u][1] (linear), then the batch sums in utterance order, and rounds the means to float32 once.
// NaN / Inf propagate as in TensorFlow: nothing is filtered.
#include "tts_common.h"

namespace tts {

namespace {

constexpr int EL_THREADS = 256;
constexpr int EL_QUADS_PER_THREAD = 8;
constexpr int EL_CHUNK = EL_THREADS * EL_QUADS_PER_THREAD * 4;   // 8192 floats = 32 KB per tensor per chunk

struct EvalLossArgs {
    const float* tgt[2];   // mel target, linear target
    const float* out[2];   // mel output, linear output
    long long n[2];        // floats per utterance slab: T * n_mels, T * F
    int nch[2];            // chunks per utterance (the same for every utterance: one more than the slab needs at most)
    int B;
    int same_align;        // output and target slabs have the same address modulo 16 bytes: 16-byte loads of both
    double* partial;       // [B * nch[0] + B * nch[1]]
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// fixed-order workgroup sum of one double per thread (EL_THREADS = 4 waves)
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();   // (lds reused across chunks)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ double quad_l1(f32x4 t, f32x4 o) {
    double s = (double)fabsf(t.x - o.x);
    s += (double)fabsf(t.y - o.y);
    s += (double)fabsf(t.z - o.z);
    s += (double)fabsf(t.w - o.w);
    return s;
}

__global__ __launch_bounds__(EL_THREADS) void eval_l1_partial_kernel(EvalLossArgs a) {
    __shared__ double lds[EL_THREADS / 64];
    const long long items0 = (long long)a.B * a.nch[0];
    const long long items = items0 + (long long)a.B * a.nch[1];
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int k = it < items0 ? 0 : 1;
        const long long r = k ? it - items0 : it;
        const long long u = r / a.nch[k];
        const long long c = r - u * a.nch[k];
        const long long n = a.n[k];
        const float* tgt = a.tgt[k] + u * n;
        const float* out = a.out[k] + u * n;
        // virtual index v = e + head: v = 0 is the 16-byte boundary at or before the slab's first float
        const int head = (int)(((uintptr_t)tgt >> 2) & 3);
        const long long v0 = c * EL_CHUNK;
        double acc = 0.0;
        if (a.same_align && v0 >= head && v0 + EL_CHUNK <= head + n) {
            // interior chunk: every quad is inside the slab and 16-byte aligned in both tensors
            const f32x4* t4 = reinterpret_cast<const f32x4*>(tgt - head + v0);
            const f32x4* o4 = reinterpret_cast<const f32x4*>(out - head + v0);
            f32x4 tv[EL_QUADS_PER_THREAD], ov[EL_QUADS_PER_THREAD];
#pragma unroll
            for (int j = 0; j < EL_QUADS_PER_THREAD; ++j) {
                tv[j] = t4[threadIdx.x + j * EL_THREADS];
                ov[j] = o4[threadIdx.x + j * EL_THREADS];
            }
#pragma unroll
            for (int j = 0; j < EL_QUADS_PER_THREAD; ++j) acc += quad_l1(tv[j], ov[j]);
        } else {
            // head / tail chunk, or an output slab aligned differently from its target: the same quads in the same order,
            // read element by element where a quad is partial or the output is misaligned
#pragma unroll 2
            for (int j = 0; j < EL_QUADS_PER_THREAD; ++j) {
                const long long e0 = v0 + 4LL * (threadIdx.x + j * EL_THREADS) - head;   // slab index of the quad's first float
                if (e0 + 4 <= 0 || e0 >= n) continue;   // (contributes +0.0: skipping it leaves the sum's bits unchanged)
                f32x4 t, o;
                if (e0 >= 0 && e0 + 4 <= n) {
                    t = *reinterpret_cast<const f32x4*>(tgt + e0);
                    if (a.same_align) {
                        o = *reinterpret_cast<const f32x4*>(out + e0);
                    } else {
                        o.x = out[e0]; o.y = out[e0 + 1]; o.z = out[e0 + 2]; o.w = out[e0 + 3];
                    }
                } else {
                    float tt[4], oo[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const long long e = e0 + q;
                        const bool in = e >= 0 && e < n;
                        tt[q] = in ? tgt[e] : 0.f;
                        oo[q] = in ? out[e] : 0.f;
                    }
                    t.x = tt[0]; t.y = tt[1]; t.z = tt[2]; t.w = tt[3];
                    o.x = oo[0]; o.y = oo[1]; o.z = oo[2]; o.w = oo[3];
                }
                acc += quad_l1(t, o);
            }
        }
        const double s = block_sum(acc, lds);
        if (threadIdx.x == 0) a.partial[it] = s;
    }
}

// one workgroup: S[u][k] = sum of utterance u's chunk partials of tensor k; then the batch means
__global__ __launch_bounds__(EL_THREADS) void eval_l1_final_kernel(const double* __restrict__ partial, int B, int nch0, int nch1,
                                                                   double cnt_mel, double cnt_lin, double* __restrict__ sums,
                                                                   float* __restrict__ losses) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items0 = (long long)B * nch0;
    for (int p = wave; p < 2 * B; p += EL_THREADS / 64) {
        const int u = p >> 1, k = p & 1;
        const int nch = k ? nch1 : nch0;
        const double* src = partial + (k ? items0 : 0) + (long long)u * nch;
        double v = 0.0;
        for (int c = lane; c < nch; c += 64) v += src[c];
        v = wave_sum(v);
        if (lane == 0) sums[p] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double dec = 0.0, post = 0.0;
        for (int u = 0; u < B; ++u) {
            dec += sums[2 * u];
            post += sums[2 * u + 1];
        }
        const float l_dec = (float)(dec / cnt_mel);
        const float l_post = (float)(post / cnt_lin);
        losses[0] = l_dec + l_post;
        losses[1] = l_dec;
        losses[2] = l_post;
    }
}

}  // namespace

size_t eval_loss_partial_count(int B, int T, int n_mels, int F) {
    const long long n0 = (long long)T * n_mels, n1 = (long long)T * F;
    return (size_t)B * (size_t)((n0 + 3 + EL_CHUNK - 1) / EL_CHUNK + (n1 + 3 + EL_CHUNK - 1) / EL_CHUNK);
}

hipError_t launch_eval_loss(hipStream_t s, const float* mel_t, const float* mel_o, const float* lin_t, const float* lin_o, int B,
                            int T, int n_mels, int F, int max_blocks, double* partial, double* sums, float* losses) {
    EvalLossArgs a;
    a.tgt[0] = mel_t;
    a.tgt[1] = lin_t;
    a.out[0] = mel_o;
    a.out[1] = lin_o;
    a.n[0] = (long long)T * n_mels;
    a.n[1] = (long long)T * F;
    for (int k = 0; k < 2; ++k) a.nch[k] = (int)((a.n[k] + 3 + EL_CHUNK - 1) / EL_CHUNK);
    a.B = B;
    a.same_align = (((uintptr_t)mel_t ^ (uintptr_t)mel_o) & 15) == 0 && (((uintptr_t)lin_t ^ (uintptr_t)lin_o) & 15) == 0;
    a.partial = partial;
    const long long items = (long long)B * (a.nch[0] + a.nch[1]);
    const int grid = (int)std::min<long long>(items, std::max(1, max_blocks));
    hipLaunchKernelGGL(eval_l1_partial_kernel, dim3(grid), dim3(EL_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eval_l1_final_kernel, dim3(1), dim3(EL_THREADS), 0, s, (const double*)partial, B, a.nch[0], a.nch[1],
                       (double)B * (double)a.n[0], (double)B * (double)a.n[1], sums, losses);
    return hipGetLastError();
}

}  // namespace tts
