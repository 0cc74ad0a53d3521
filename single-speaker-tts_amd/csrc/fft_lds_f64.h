// The double twin of fft_lds.h's glg_fft, for stoi.hip: a scalar complex double type and the in-place radix-4 / radix-2 forward
// transform of several frames of M = 1 << MM points at once, on bit-reversed input in LDS.  fft_lds.h stays as it is.
#pragma once
#include "tts_common.h"

namespace tts {

// A complex number as two SCALAR doubles (fft_lds.h has the history of the scalar form; there is no packed f64 arithmetic).
struct __attribute__((aligned(16))) dcf { double x, y; };
__device__ __forceinline__ dcf operator+(dcf a, dcf b) { return dcf{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ dcf operator-(dcf a, dcf b) { return dcf{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ dcf dmul(dcf a, dcf b) { return (dcf){a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ dcf dmul_mi(dcf a) { return (dcf){a.y, -a.x}; }    // -i a

// In-place decimation-in-time forward FFT of `frames` arrays of M = 1 << MM complex values, array f at a + f * M, each ALREADY
// in bit-reversed order.  tw[TWS k] = exp(-2 pi i k / M), k < M / 2 (TWS = 2: the table of a transform twice as long, which a
// real transform of 2 M points needs for its last step anyway).  Two radix-2 stages per pass, as in glg_fft: the four values
// (base + q half, q < 4) of a radix-4 group go through stage s (one twiddle) and stage s + 1 (twiddles w and -i w) in registers;
// a last single stage when MM is odd.  All lanes of the workgroup take part (barriers); `frames` is uniform.
template <int MM, int TWS>
__device__ __forceinline__ void fft_f64_lds(dcf* a, const dcf* __restrict__ tw, int frames) {
    constexpr int M = 1 << MM;
    int s = 1;
    for (; s + 1 <= MM; s += 2) {
        const int half = 1 << (s - 1);
        __syncthreads();
        for (int g = threadIdx.x; g < frames * (M / 4); g += blockDim.x) {
            const int f = g / (M / 4), i = g % (M / 4);
            const int j = i & (half - 1);
            dcf* p = a + (size_t)f * M + (((i - j) << 2) + j);
            const dcf w1 = tw[(j << (MM - s)) * TWS];      // stage s:     W_M^(j M / 2^s)
            const dcf w2 = tw[(j << (MM - s - 1)) * TWS];    // stage s + 1: W_M^(j M / 2^(s+1)); its partner at j + half is -i times that
            const dcf x0 = p[0], x1 = dmul(p[half], w1), x2 = p[2 * half], x3 = dmul(p[3 * half], w1);
            const dcf u0 = x0 + x1, u1 = x0 - x1, u2 = dmul(x2 + x3, w2);
            const dcf u3 = dmul_mi(dmul(x2 - x3, w2));
            p[0] = u0 + u2;
            p[half] = u1 + u3;
            p[2 * half] = u0 - u2;
            p[3 * half] = u1 - u3;
        }
    }
    if (s == MM) {   // one radix-2 stage left
        const int half = 1 << (s - 1);
        __syncthreads();
        for (int g = threadIdx.x; g < frames * (M / 2); g += blockDim.x) {
            const int f = g / (M / 2), i = g % (M / 2);
            const int j = i & (half - 1);
            dcf* p = a + (size_t)f * M + (((i - j) << 1) + j);
            const dcf w = tw[(j << (MM - s)) * TWS];
            const dcf u = p[0], v = dmul(p[half], w);
            p[0] = u + v;
            p[half] = u - v;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int fft_f64_bitrev(int i, int m) { return (int)(__brev((unsigned)i) >> (32 - m)); }

}  // namespace tts
