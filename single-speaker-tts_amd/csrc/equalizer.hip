// The equaliser: a cascade of up to 8 second-order sections over batches of mono waveforms -- loudness.hip's K-weighting recurrence
// in its general form, with the output written.  No reference counterpart.  include/sstts_hip.h has the definition in full and
// equalizer_plan.h the cut and the order of every operation; every product and sum is an individually rounded IEEE double
// operation, so the results are the bits of tests/equalizer_oracle.py.
//
// The recurrence is sequential, so a row is cut into segments of EQ_SEG = 256 samples and a lane owns a segment:
//   eq_transition_kernel   the 2 S x 2 S transition of a segment, by the recurrence itself: lane j runs from the unit state j
//   eq_segments_kernel<0>  the cascade over every segment but the row's last from the zero state; keeps the state it ends in
//   eq_chain_kernel        one wave per utterance chains those states: lane r owns row r of the transition and value r of the state
//   eq_segments_kernel<1>  every segment again from its initial state; each y rounded to float32 once and written
// Neighbouring lanes sit a segment apart, so a workgroup (one wave) stages a tile of 64 segments through LDS: the tile travels
// between memory and LDS in 16-byte accesses of neighbouring lanes (a wave moves 1 KB of a row per access; the up to three floats
// in front of the first aligned address and behind the last go one by one), and lane l walks row l of the tile, rows 257 floats
// apart: at step i the lanes read banks (l + i) mod 32, all different within each half of the wave.  Pass 3 writes its output back
// into the tile it read.  A tile is 64.25 KB, two fit a compute unit: the passes are bound by the dependent double chain of a lane at
// that occupancy, not by memory.
// No atomics; every loop bound is a host value that travelled in the launch.
#include "api_internal.h"
#include "equalizer_plan.h"
#include "equalizer_tile.h"

// y = b0 x + z1 is a product and a sum (tests/equalizer_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct EqLens {
    int n[EQ_UTTS];
};

struct EqCoef {
    double k[5 * EQ_MAX_SECTIONS];
};

// One section-unrolled sample (eq_sample with S a compile-time value: the state stays in registers).
template <int S>
__device__ __forceinline__ double eq_step(const EqCoef& c, double (&st)[2 * S], double x) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double y = c.k[5 * s] * x + st[2 * s];
        st[2 * s] = (c.k[5 * s + 1] * x - c.k[5 * s + 3] * y) + st[2 * s + 1];
        st[2 * s + 1] = c.k[5 * s + 2] * x - c.k[5 * s + 4] * y;
        x = y;
    }
    return x;
}

// M[r][j], row-major 2 S x 2 S: lane j runs EQ_SEG samples of zero input from the unit state j.
template <int S>
__global__ __launch_bounds__(EQ_LANES) void eq_transition_kernel(EqCoef coef, double* __restrict__ M) {
    const int j = threadIdx.x;
    if (j >= 2 * S) return;
    double st[2 * S];
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) st[r] = r == j ? 1.0 : 0.0;
    for (int i = 0; i < EQ_SEG; ++i) eq_step<S>(coef, st, 0.0);
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) M[2 * S * r + j] = st[r];
}

// wav (and out, PASS 1) point at the first utterance of the launch, rows `row` floats apart; state at its states, state_row
// doubles apart: [2 S][segs] with segs = eq_segments(row).  PASS 0: from the zero state, the end state kept; PASS 1: from the state
// kept there by the chain, the output written.
template <int S, int PASS>
__global__ __launch_bounds__(EQ_LANES) void eq_segments_kernel(const float* wav, float* out /* may equal wav */, size_t row, EqLens lens,
                                                               EqCoef coef, double* __restrict__ state, size_t state_row, size_t segs) {
    extern __shared__ float eq_tile[];
    const int b = blockIdx.y, lane = threadIdx.x;
    const long long n = lens.n[b];
    const long long first = (long long)blockIdx.x * EQ_TILE;
    const long long n_seg = eq_segments(n);
    // (uniform) nothing of this row in the tile -- or, in pass 0, only its last segment, whose end state nobody reads
    if (first >= n || (PASS == 0 && (long long)blockIdx.x * EQ_TILE_SEGS >= n_seg - 1)) return;
    const int count = (int)min((long long)EQ_TILE, n - first);
    eq_move_tile<true>(const_cast<float*>(wav) + (size_t)b * row, first, count, eq_tile, lane);
    __syncthreads();
    const long long seg = (long long)blockIdx.x * EQ_TILE_SEGS + lane;
    const bool mine = PASS == 0 ? seg < n_seg - 1 : seg < n_seg;
    if (mine) {
        const int len = eq_segment_len(n, seg);
        double* sp = state + (size_t)b * state_row + (size_t)seg;
        double st[2 * S];
#pragma unroll
        for (int r = 0; r < 2 * S; ++r) st[r] = PASS == 0 ? 0.0 : sp[(size_t)r * segs];
        float* t = eq_tile + lane * EQ_LDS_STRIDE;
        if (len == EQ_SEG) {
#pragma unroll 8
            for (int i = 0; i < EQ_SEG; ++i) {
                const double y = eq_step<S>(coef, st, (double)t[i]);
                if (PASS == 1) t[i] = (float)y;
            }
        } else {
            for (int i = 0; i < len; ++i) {
                const double y = eq_step<S>(coef, st, (double)t[i]);
                if (PASS == 1) t[i] = (float)y;
            }
        }
        if (PASS == 0) {
#pragma unroll
            for (int r = 0; r < 2 * S; ++r) sp[(size_t)r * segs] = st[r];
        }
    }
    if (PASS == 1) {
        __syncthreads();
        eq_move_tile<false>(out + (size_t)b * row, first, count, eq_tile, lane);
    }
}

// In place: the end states of pass 0 become the segments' initial states.  One wave per utterance; lane r < 2 S owns row r of the
// transition and value r of the state, and takes the other values from its neighbours.  The next segment's end state is loaded
// while this link runs.
template <int S>
__global__ __launch_bounds__(EQ_LANES) void eq_chain_kernel(EqLens lens, const double* __restrict__ M, double* __restrict__ state, size_t state_row,
                                                            size_t segs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool active = lane < 2 * S;
    const int r = active ? lane : 0;
    const long long n_seg = eq_segments((long long)lens.n[b]);
    double* sp = state + (size_t)b * state_row + (size_t)r * segs;
    double m[2 * S];
#pragma unroll
    for (int j = 0; j < 2 * S; ++j) m[j] = M[2 * S * r + j];
    double Sr = 0.0;
    double e_next = n_seg > 1 ? sp[0] : 0.0;
    for (long long i = 0; i < n_seg; ++i) {
        const double e = e_next;
        if (i + 2 < n_seg) e_next = sp[i + 1];
        if (active) sp[i] = Sr;
        double a = __dmul_rn(m[0], __shfl(Sr, 0, 64));
#pragma unroll
        for (int j = 1; j < 2 * S; ++j) a = __dadd_rn(a, __dmul_rn(m[j], __shfl(Sr, j, 64)));
        Sr = __dadd_rn(a, e);
    }
}

}  // namespace tts

namespace tts_api {

template <int S>
static void eq_launch_transition(hipStream_t stream, const EqCoef& coef, double* M) {
    hipLaunchKernelGGL(eq_transition_kernel<S>, dim3(1), dim3(EQ_LANES), 0, stream, coef, M);
}

template <int S>
static hipError_t eq_launch_chunk(hipStream_t stream, const float* wav, float* out, size_t row, const EqLens& lens, int nb, int longest,
                                  const EqCoef& coef, const double* M, double* state, size_t state_row, size_t segs) {
    const size_t lds = eq_lds_bytes();   // (over 64 KB: asked for by name, as limiter.hip does)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eq_segments_kernel<S, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eq_segments_kernel<S, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)eq_tiles(longest), nb);
    hipLaunchKernelGGL((eq_segments_kernel<S, 0>), grid, dim3(EQ_LANES), lds, stream, wav, out, row, lens, coef, state, state_row, segs);
    hipLaunchKernelGGL(eq_chain_kernel<S>, dim3(nb), dim3(EQ_LANES), 0, stream, lens, M, state, state_row, segs);
    hipLaunchKernelGGL((eq_segments_kernel<S, 1>), grid, dim3(EQ_LANES), lds, stream, wav, out, row, lens, coef, state, state_row, segs);
    return hipGetLastError();
}

// The workspaces of a tts_equalize call on B rows of N samples through n_sections sections.
int equalizer_scratch(tts_handle_t h, int B, int N, int n_sections, EqScratch* s) {
    WS(h, "eq.state", double, (size_t)B * eq_state_doubles(N, n_sections), state);
    WS(h, "eq.M", double, eq_transition_doubles(n_sections), M);
    *s = EqScratch{state, M};
    return TTS_OK;
}

#define EQ_BY_SECTIONS(S, call)          \
    switch (S) {                         \
        case 1: call(1); break;          \
        case 2: call(2); break;          \
        case 3: call(3); break;          \
        case 4: call(4); break;          \
        case 5: call(5); break;          \
        case 6: call(6); break;          \
        case 7: call(7); break;          \
        default: call(8); break;         \
    }

// On h->stream; everything has been checked (equalizer_check).
int equalizer_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const double* sos, int n_sections) {
    EqScratch s;
    const int rc = equalizer_scratch(h, B, N, n_sections, &s);
    if (rc) return rc;
    EqCoef coef;
    for (int i = 0; i < 5 * EQ_MAX_SECTIONS; ++i) coef.k[i] = i < 5 * n_sections ? sos[i] : 0.0;
    const size_t segs = (size_t)eq_segments(N), state_row = eq_state_doubles(N, n_sections);
    ProfScope ps(h, ST_EQUALIZE, (int64_t)length_chunks(B, EQ_UTTS) * 3 + 1);
#define EQ_TRANSITION(S) eq_launch_transition<S>(h->stream, coef, s.M)
    EQ_BY_SECTIONS(n_sections, EQ_TRANSITION)
#undef EQ_TRANSITION
    HIPCHK(h, hipGetLastError());
    for (int b0 = 0; b0 < B; b0 += EQ_UTTS) {
        const int nb = std::min(EQ_UTTS, B - b0);
        EqLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        hipError_t e = hipSuccess;
#define EQ_CHUNK(S) \
    e = eq_launch_chunk<S>(h->stream, wav + (size_t)b0 * N, out + (size_t)b0 * N, (size_t)N, lens, nb, longest, coef, s.M, s.state + (size_t)b0 * state_row, state_row, segs)
        EQ_BY_SECTIONS(n_sections, EQ_CHUNK)
#undef EQ_CHUNK
        HIPCHK(h, e);
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_equalizer_max_sections(void) { return EQ_MAX_SECTIONS; }

int tts_equalizer_design(int kind, int sampling_rate, double f0_hz, double q, double gain_db, double* sos5_out) {
    if (!sos5_out) return TTS_ERR_INVALID;
    bool invalid = false;
    const std::string why = eq_design(kind, sampling_rate, f0_hz, q, gain_db, sos5_out, &invalid);
    return why.empty() ? TTS_OK : invalid ? TTS_ERR_INVALID : TTS_ERR_UNSUPPORTED;
}

int tts_equalizer_profile(const char* name, int sampling_rate, double* sos_out, int* n_sections_out) {
    bool invalid = false;
    double sos[5 * EQ_MAX_SECTIONS];
    int n = 0;
    const std::string why = eq_profile(name, sampling_rate, sos_out ? sos : nullptr, &n, &invalid);
    if (!why.empty()) return fail(nullptr, invalid ? TTS_ERR_INVALID : TTS_ERR_UNSUPPORTED, "equalizer_profile: " + why);
    for (int i = 0; i < 5 * n; ++i) sos_out[i] = sos[i];
    *n_sections_out = n;
    return TTS_OK;
}

int tts_equalize(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const double* sos, int n_sections) {
    DeviceScope dev_scope(h);
    const std::string why = equalizer_check(reinterpret_cast<uintptr_t>(wav), reinterpret_cast<uintptr_t>(out), B, N, n_samples, sos, n_sections);
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "equalize: " + why);
    if (!h) return TTS_ERR_INVALID;
    return equalizer_impl(h, wav, out, B, N, n_samples, sos, n_sections);
}

int tts_set_equalizer(tts_handle_t h, int enabled, const double* sos, int n_sections) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled) {
        const std::string why = sos ? eq_sections_check(sos, n_sections) : std::string("a NULL pointer (sos is required)");
        if (!why.empty()) return fail(h, TTS_ERR_INVALID, "set_equalizer: " + why);
        for (int i = 0; i < 5 * n_sections; ++i) h->settings.eq.sos[i] = sos[i];
        h->settings.eq.n_sections = n_sections;
    }
    h->settings.eq.enabled = enabled != 0;
    return TTS_OK;
}

}  // extern "C"
