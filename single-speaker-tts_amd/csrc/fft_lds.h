// The LDS FFT of griffin_lim_generic.hip, shared with features.hip: scalar complex type and the in-place radix-4 / radix-2
// transform of any power-of-two size on bit-reversed input.  Files that include this are built with -fno-slp-vectorize
// (build.py; see the note on gcf).
#pragma once
#include "tts_common.h"

namespace tts {


// A complex number as two SCALAR floats, and the file is built with -fno-slp-vectorize (build.py): no v_pk_*_f32 instruction is
// selected for these kernels.  Round 6 measured why (profiles/r06_experiment_packed_f32_beside_mfma.txt): written with a float2
// vector type the compiler made the butterflies from packed-f32 VOP3P instructions, and whenever waves of the MFMA GEMM
// (gemm_f32_kernel, another stream) shared the compute unit, single frames came out wrong -- the low dword of a packed result in
// lanes 48-63 of one wave, as stored to LDS by the next instruction: 129 of 200 calls beside GEMM launches, 0 of 3100 for the
// same source without packed selection (and 0 of 120 for every other stage of the library under the same neighbour).  The
// kernels are bound by memory: the scalar form costs nothing (926 / 523 us per iteration at n_fft 2048 / 1024 either way).
struct __attribute__((aligned(8))) gcf { float x, y; };
__device__ __forceinline__ gcf operator+(gcf a, gcf b) { return gcf{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ gcf operator-(gcf a, gcf b) { return gcf{a.x - b.x, a.y - b.y}; }

__device__ __forceinline__ gcf gmul(gcf a, gcf b) { return (gcf){a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

__device__ __forceinline__ gcf gconj(gcf a) { return (gcf){a.x, -a.y}; }
__device__ __forceinline__ gcf gmul_i(gcf a) { return (gcf){-a.y, a.x}; }     // i a
__device__ __forceinline__ gcf gmul_mi(gcf a) { return (gcf){a.y, -a.x}; }    // -i a

// In-place decimation-in-time FFT of `a`: M = 1 << mm complex values in LDS, ALREADY in bit-reversed order.  tw[k] =
// exp(-2 pi i k / (2 M)), k < M (the table of the real transform of 2 M points): W_M^j = tw[2 j].  INVERSE conjugates the
// twiddles (no 1 / M scale).  Two radix-2 stages per pass: the four values (base + q half, q < 4) of a radix-4 group go through
// stage s (pairs (0,1), (2,3), one twiddle) and stage s + 1 (pairs (0,2), (1,3), twiddles w and -i w) in registers; a last single
// stage when mm is odd.
template <bool INVERSE>
__device__ __forceinline__ void glg_fft(gcf* a, const gcf* __restrict__ tw, int M, int mm) {
    int s = 1;
    for (; s + 1 <= mm; s += 2) {
        const int half = 1 << (s - 1);
        __syncthreads();
        for (int i = threadIdx.x; i < M / 4; i += blockDim.x) {
            const int j = i & (half - 1);
            const int base = ((i - j) << 2) + j;
            gcf w1 = tw[(j << (mm - s)) << 1];          // stage s:     W_M^(j M / 2^s)
            gcf w2 = tw[(j << (mm - s - 1)) << 1];      // stage s + 1: W_M^(j M / 2^(s+1)); its partner at j + half is -i (forward) times that
            if (INVERSE) { w1.y = -w1.y; w2.y = -w2.y; }
            const gcf x0 = a[base], x1 = gmul(a[base + half], w1), x2 = a[base + 2 * half], x3 = gmul(a[base + 3 * half], w1);
            const gcf u0 = x0 + x1, u1 = x0 - x1, u2 = gmul(x2 + x3, w2);
            const gcf t3 = gmul(x2 - x3, w2);
            const gcf u3 = INVERSE ? gmul_i(t3) : gmul_mi(t3);
            a[base] = u0 + u2;
            a[base + half] = u1 + u3;
            a[base + 2 * half] = u0 - u2;
            a[base + 3 * half] = u1 - u3;
        }
    }
    if (s == mm) {   // one radix-2 stage left
        const int half = 1 << (s - 1);
        __syncthreads();
        for (int i = threadIdx.x; i < M / 2; i += blockDim.x) {
            const int j = i & (half - 1);
            const int base = ((i - j) << 1) + j;
            gcf w = tw[(j << (mm - s)) << 1];
            if (INVERSE) w.y = -w.y;
            const gcf u = a[base], v = gmul(a[base + half], w);
            a[base] = u + v;
            a[base + half] = u - v;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int glg_bitrev(int i, int m) { return (int)(__brev((unsigned)i) >> (32 - m)); }

}  // namespace tts
