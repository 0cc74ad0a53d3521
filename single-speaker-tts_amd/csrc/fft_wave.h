// Wave-level FFT building blocks of griffin_lim.hip, shared with features.hip: packed complex helpers, the radix-4 / 16
// butterflies and the one-wave 1024-point complex FFT (16 points per lane).  Index math: see griffin_lim.hip's header and
// tests/test_host_logic.py (test_fft_decomposition_emulation).  Files that include this are built with -fno-slp-vectorize
// (build.py): the packed instructions here are written out explicitly, nothing else is packed.
//
// FFT_WAVE_SCALAR (defined before the include): the same transforms with a complex number as two SCALAR floats and every
// helper in plain scalar arithmetic, so that no v_pk_*_f32 instruction is selected -- the form of griffin_lim_generic.hip,
// whose packed results were stored wrong beside MFMA waves of another stream (see the note on gcf in fft_lds.h).  Its symbols
// live in the inline namespace tts::fft_scalar, apart from the packed ones.
#pragma once
#include "tts_common.h"
#include "gl_plan.h"   // EX_CPLX

#ifdef FFT_WAVE_SCALAR
namespace tts {
inline namespace fft_scalar {
struct __attribute__((aligned(8))) cf { float x, y; };
__device__ __forceinline__ cf cmk(float a, float b) { return cf{a, b}; }
__device__ __forceinline__ cf cadd(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf cscale(cf a, float s) { return cf{a.x * s, a.y * s}; }
__device__ __forceinline__ cf cconj(cf a) { return cf{a.x, -a.y}; }
__device__ __forceinline__ cf cadd_mi(cf a, cf b) { return cf{a.x + b.y, a.y - b.x}; }
__device__ __forceinline__ cf cadd_pi(cf a, cf b) { return cf{a.x - b.y, a.y + b.x}; }
__device__ __forceinline__ cf cconj_add_pi(cf a, cf b) { return cf{a.x - b.y, -a.y - b.x}; }
__device__ __forceinline__ cf cconj_sub(cf a, cf b) { return cf{a.x - b.x, -a.y + b.y}; }
__device__ __forceinline__ cf cadd_conj(cf a, cf b) { return cf{a.x + b.x, a.y - b.y}; }
__device__ __forceinline__ cf csub_conj(cf a, cf b) { return cf{a.x - b.x, a.y + b.y}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return cf{fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y)}; }
__device__ __forceinline__ cf cmul_conj(cf a, cf b) { return cf{fmaf(a.y, b.y, a.x * b.x), fmaf(a.y, b.x, -(a.x * b.y))}; }
__device__ __forceinline__ cf cmul_k(cf a, cf k) { return cmul(a, k); }
__device__ __forceinline__ cf cneg_add_mi(cf a, cf b) { return cf{-a.x + b.y, -a.y - b.x}; }
__device__ __forceinline__ cf cneg_add_pi(cf a, cf b) { return cf{-a.x - b.y, -a.y + b.x}; }
#else
namespace tts {
inline namespace fft_packed {
typedef float cf __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf cmk(float a, float b) { return (cf){a, b}; }
__device__ __forceinline__ cf cadd(cf a, cf b) { return a + b; }
__device__ __forceinline__ cf csub(cf a, cf b) { return a - b; }
__device__ __forceinline__ cf cscale(cf a, float s) { return a * s; }
__device__ __forceinline__ cf cconj(cf a) { return cmk(a.x, -a.y); }
// a + (-i) b = (a.x + b.y, a.y - b.x)
__device__ __forceinline__ cf cadd_mi(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + (+i) b = (a.x - b.y, a.y + b.x)
__device__ __forceinline__ cf cadd_pi(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// conj(a + i b) = (a.x - b.y, -a.y - b.x)
__device__ __forceinline__ cf cconj_add_pi(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// conj(a - b) = (a.x - b.x, -a.y + b.y)
__device__ __forceinline__ cf cconj_sub(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + conj(b), a - conj(b)
__device__ __forceinline__ cf cadd_conj(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf csub_conj(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a * b
__device__ __forceinline__ cf cmul(cf a, cf b) {
    cf t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
// a * conj(b) = (a.x b.x + a.y b.y, a.y b.x - a.x b.y)
__device__ __forceinline__ cf cmul_conj(cf a, cf b) {
    cf t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}
// a * k for a compile-time constant k, which lives in a scalar register pair
__device__ __forceinline__ cf cmul_k(cf a, cf k) {
    cf t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "s"(k));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "s"(k), "v"(t));
    return r;
}
// -a - i b = (-a.x + b.y, -a.y - b.x) and -a + i b = (-a.x - b.y, -a.y + b.x)
__device__ __forceinline__ cf cneg_add_mi(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[1,0] neg_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf cneg_add_pi(cf a, cf b) {
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[1,1] neg_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
#endif


// ------------------------------------------------------------------------------------ complex helpers
// A complex number is ONE packed value (an aligned 64-bit register pair): gfx950 issues a VALU instruction per
// wave every ~4 cycles whether it is v_add_f32 or v_pk_add_f32 (tools/valu_microbench2.hip: 1.72 ns against
// 1.84 ns per instruction and SIMD), so complex add / sub cost one instruction and a complex multiply two
// (v_pk_mul_f32 + v_pk_fma_f32).  Multiplications by +-i, conjugations and the real / imaginary broadcasts of
// the multiply are the op_sel / neg_lo / neg_hi source modifiers of the packed instructions; hipcc does not
// form those from shuffles (it emits v_mov + v_xor), hence the one-line asm statements.  Plain asm, not
// volatile: the compiler still schedules and removes them like any other pure operation.
__device__ __forceinline__ void wave_lds_sync() {
    // LDS hand-off between lanes of ONE wave.  The LDS unit executes one wave's DS operations in
    // issue order, so a ds_read issued after a ds_write of the same wave observes it for every
    // lane: no s_waitcnt is needed, only a compiler-level ordering point (the compiler still waits
    // on lgkmcnt before it USES a loaded register).
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// forward radix-4 butterfly (W4 = -i): 8 packed adds
__device__ __forceinline__ void r4(cf& a, cf& b, cf& c, cf& d) {
    const cf s0 = cadd(a, c), s1 = csub(a, c), s2 = cadd(b, d), s3 = csub(b, d);
    a = cadd(s0, s2);
    c = csub(s0, s2);
    b = cadd_mi(s1, s3);   // a - i b - c + i d
    d = cadd_pi(s1, s3);   // a + i b - c - i d
}
// the same with c standing for (-i) c: the W16^4 twiddle of the 16-point transform folded into the butterfly
__device__ __forceinline__ void r4_c_mi(cf& a, cf& b, cf& c, cf& d) {
    const cf s0 = cadd_mi(a, c), s1 = cadd_pi(a, c), s2 = cadd(b, d), s3 = csub(b, d);
    a = cadd(s0, s2);
    c = csub(s0, s2);
    b = cadd_mi(s1, s3);
    d = cadd_pi(s1, s3);
}

// The radix-4 butterfly with inputs KNOWN to be zero (ZA: a, ZD: d): the frame a forward transform is fed is zero outside
// the window's 128-sample slots, i.e. in the first and last registers of a lane (fft_input), and x + 0 is not something
// the compiler may drop (-0 + 0 = +0), let alone through the asm statements.  6 packed adds with one zero, 4 with two.
template <bool ZA, bool ZD>
__device__ __forceinline__ void r4z(cf& a, cf& b, cf& c, cf& d) {
    if (ZA && ZD) {          // s0 = c, s1 = -c, s2 = s3 = b
        const cf b0 = b, c0 = c;
        a = cadd(c0, b0);
        c = csub(c0, b0);
        b = cneg_add_mi(c0, b0);
        d = cneg_add_pi(c0, b0);
    } else if (ZA) {         // s0 = c, s1 = -c
        const cf c0 = c, s2 = cadd(b, d), s3 = csub(b, d);
        a = cadd(c0, s2);
        c = csub(c0, s2);
        b = cneg_add_mi(c0, s3);
        d = cneg_add_pi(c0, s3);
    } else if (ZD) {         // s2 = s3 = b
        const cf b0 = b, s0 = cadd(a, c), s1 = csub(a, c);
        a = cadd(s0, b0);
        c = csub(s0, b0);
        b = cadd_mi(s1, b0);
        d = cadd_pi(s1, b0);
    } else {
        r4(a, b, c, d);
    }
}

// forward 16-point DFT in registers, natural order in and out: out[k] = sum_j v[j] W16^{jk}
// (64 packed adds + 8 complex multiplies by constants = 80 VALU instructions).  ZLO / ZHI: the inputs v[j], j < ZLO or
// j > ZHI, are known to be zero (their registers are not read): the reference window's [3, 12] saves 12 of the 32 adds of step 1
template <int ZLO = 0, int ZHI = 15>
__device__ __forceinline__ void fft16(cf (&v)[16]) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    // step 1: for each j1, radix-4 over j2 (elements j1 + 4 j2) -> t[j1][k2] stored at v[j1 + 4 k2]
    {
        // (only the two patterns r4z knows are used: a zero first and / or last input, the middle two present)
        constexpr bool ok = ZLO >= 0 && ZLO <= 4 && ZHI >= 11 && ZHI <= 15;
        static_assert(ok || (ZLO == 0 && ZHI == 15), "fft16: zero inputs in the first and last four registers only");
        r4z<(0 < ZLO), (12 > ZHI)>(v[0], v[4], v[8], v[12]);
        r4z<(1 < ZLO), (13 > ZHI)>(v[1], v[5], v[9], v[13]);
        r4z<(2 < ZLO), (14 > ZHI)>(v[2], v[6], v[10], v[14]);
        r4z<(3 < ZLO), (15 > ZHI)>(v[3], v[7], v[11], v[15]);
    }
    // twiddle t[j1][k2] *= W16^{j1 k2}; W^4 = -i (t[2][2]) is folded into the second butterfly of k2 = 2
    v[1 + 4] = cmul_k(v[1 + 4], cmk(C1, -S1));    // W^1
    v[1 + 8] = cmul_k(v[1 + 8], cmk(R2, -R2));    // W^2
    v[1 + 12] = cmul_k(v[1 + 12], cmk(S1, -C1));  // W^3
    v[2 + 4] = cmul_k(v[2 + 4], cmk(R2, -R2));    // W^2
    v[2 + 12] = cmul_k(v[2 + 12], cmk(-R2, -R2)); // W^6
    v[3 + 4] = cmul_k(v[3 + 4], cmk(S1, -C1));    // W^3
    v[3 + 8] = cmul_k(v[3 + 8], cmk(-R2, -R2));   // W^6
    v[3 + 12] = cmul_k(v[3 + 12], cmk(-C1, S1));  // W^9
    // step 2: for each k2, radix-4 over j1 -> out[k2 + 4 k1] ; data for k2 sits at v[4 k2 + j1]
    cf o[16];
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
        cf a = v[4 * k2 + 0], b = v[4 * k2 + 1], c = v[4 * k2 + 2], d = v[4 * k2 + 3];
        if (k2 == 2) r4_c_mi(a, b, c, d);
        else r4(a, b, c, d);
        o[k2 + 0] = a; o[k2 + 4] = b; o[k2 + 8] = c; o[k2 + 12] = d;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = o[i];
}

#define E2S 17
static_assert(EX_CPLX >= 64 * E2S && EX_CPLX > 1024, "a wave's exchange buffer: 64 rows of E2S (the only exchange image), and the 1024 bins + Nyquist of the merge pass");

struct FftTw {
    const cf* a;   // LDS table: a[(k2-1)*64] = W1024^{lane*k2}, k2 = 1..15 (already offset by lane)
    cf b[3];       // W64^{(lane&15)*d}, d = 1..3
    __device__ __forceinline__ cf a_at(int k2) const { return a[(k2 - 1) * 64]; }
};
struct FftTwReg {  // the same twiddles held in registers for the whole kernel (no LDS reads inside the FFT)
    cf a[15];
    cf b[3];
    __device__ __forceinline__ cf a_at(int k2) const { return a[k2 - 1]; }
};

// forward 1024-point complex FFT across one wave.  in: v[j] = z[lane + 64 j]; out: v[c] = Z[lane + 64 c].
// Exchange a register-index bit with a lane-index bit, for the pair of complex registers (a, b):
// v_permlane32_swap / v_permlane16_swap transpose the 2 x 2 block {a, b} x {lane bit 5 (or 4) = 0, 1}:
// afterwards a holds [a.lo | b.lo] and b holds [a.hi | b.hi] (halves of 32 lanes, or rows of 16).
__device__ __forceinline__ void swap_bit5(cf& a, cf& b) {
    auto rx = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
    auto ry = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
    a = cmk(__uint_as_float(rx[0]), __uint_as_float(ry[0]));
    b = cmk(__uint_as_float(rx[1]), __uint_as_float(ry[1]));
}
__device__ __forceinline__ void swap_bit4(cf& a, cf& b) {
    auto rx = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
    auto ry = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
    a = cmk(__uint_as_float(rx[0]), __uint_as_float(ry[0]));
    b = cmk(__uint_as_float(rx[1]), __uint_as_float(ry[1]));
}

// forward 1024-point complex FFT across one wave.  in: v[j] = z[lane + 64 j]; out: v[c] = Z[lane + 64 c].
// Index split n = lane + 64 j, k = k2 + 16 k1', ...: radix-16 over j in registers, twiddle, then the
// element (row k2, column lane) has to reach lane (a = lane & 15, kq = k2 & 3) register (k2 >> 2, lane >> 4):
// a 4 x 4 transpose between the two low register-index bits and the two high lane bits, done with
// 32 permlane swaps (no LDS); radix-4; the second exchange (a 16 x 16 transpose inside each row of 16
// lanes) goes through the wave's LDS buffer; radix-16.
template <int ZLO = 0, int ZHI = 15, typename TW>
__device__ __forceinline__ void fft1024(cf (&v)[16], cf* ex, const TW& tw, int lane) {
    fft16<ZLO, ZHI>(v);
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) v[k2] = cmul(v[k2], tw.a_at(k2));
    // new v[4 i + b] at lane (a, kq) = old v[4 i + kq] at lane (a, b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        swap_bit4(v[4 * i + 0], v[4 * i + 1]);
        swap_bit4(v[4 * i + 2], v[4 * i + 3]);
        swap_bit5(v[4 * i + 0], v[4 * i + 2]);
        swap_bit5(v[4 * i + 1], v[4 * i + 3]);
    }
    const int a = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
#pragma unroll
        for (int d = 1; d < 4; ++d) v[4 * i + d] = cmul(v[4 * i + d], tw.b[d - 1]);
#pragma unroll
        for (int d = 0; d < 4; ++d) ex[(16 * d + kq + 4 * i) * E2S + a] = v[4 * i + d];
    }
    wave_lds_sync();
#pragma unroll
    for (int x = 0; x < 16; ++x) v[x] = ex[lane * E2S + x];
    wave_lds_sync();
    fft16(v);
}


}  // inline namespace
}  // namespace tts
