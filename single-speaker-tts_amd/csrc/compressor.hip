// The dynamics compressor: a feed-forward peak compressor over batches of mono waveforms.  No reference counterpart.
// include/sstts_hip.h has the definition in full and compressor_plan.h the cut and the order of every operation; the detector is
// individually rounded IEEE double operations, so the envelope is the bits of tests/compressor_oracle.py; the gain goes through
// log10 and pow and is held to a bound.
//
// Both recurrences are sequential and the first is not linear, so a row is cut into the equaliser's segments of EQ_SEG = 256 samples
// and a lane owns a segment:
//   cmp_segments_kernel<0>  (A) the release follower over every segment but the row's last from 0; keeps c, the e1 it ends in
//   cmp_chain_kernel<0>     one wave per utterance: s[k+1] = max(c[k], AR s[k]), 64 links a load
//   cmp_segments_kernel<1>  (B) every segment but the last again from its true e1 and from e = 0; keeps q, the e it ends in
//   cmp_chain_kernel<1>     t[k+1] = AA t[k] + q[k]
//   cmp_segments_kernel<2>  (C) every segment from both true states: the gain, the output rounded to float32 once
//   cmp_stats_kernel        (only where records are asked for) a row's record out of pass C's one partial a tile
// The tile of 64 segments travels through LDS as the equaliser's does (equalizer_tile.h); pass C writes its output back into the
// tile it read.  No atomics; every loop bound is a host value that travelled in the launch.
#include "api_internal.h"
#include "compressor_plan.h"
#include "equalizer_tile.h"

// e = aA e + bA e1 is two products and a sum (tests/compressor_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct CmpLens {
    int n[CMP_UTTS];
};

// what pass C knows of a tile of one row
struct CmpPartial {
    int reduced;
    float peak;
    double max_reduction;
};
static_assert(sizeof(CmpPartial) == 16 && sizeof(tts_compress_stats_t) == 16, "16-byte records");

// wav (and out, PASS 2) point at the first utterance of the launch, rows `row` floats apart; state at its states, state_row doubles
// apart: [2][segs], c -> s in front and q -> t behind.  envelope and partial: pass C's optional outputs (or null).
template <int PASS>
__global__ __launch_bounds__(EQ_LANES) void cmp_segments_kernel(const float* wav, float* out /* may equal wav */, size_t row, CmpLens lens, CmpCoef k,
                                                                double* __restrict__ state, size_t state_row, size_t segs,
                                                                double* __restrict__ envelope, CmpPartial* __restrict__ partial, size_t partial_row) {
    extern __shared__ float cmp_tile[];
    const int b = blockIdx.y, lane = threadIdx.x;
    const long long n = lens.n[b];
    const long long first = (long long)blockIdx.x * EQ_TILE;
    const long long n_seg = eq_segments(n);
    // (uniform) nothing of this row in the tile -- or, in passes A and B, only its last segment, whose end state nobody reads
    if (first >= n || (PASS < 2 && (long long)blockIdx.x * EQ_TILE_SEGS >= n_seg - 1)) return;
    const int count = (int)min((long long)EQ_TILE, n - first);
    eq_move_tile<true>(const_cast<float*>(wav) + (size_t)b * row, first, count, cmp_tile, lane);
    __syncthreads();
    const long long seg = (long long)blockIdx.x * EQ_TILE_SEGS + lane;
    const bool mine = PASS < 2 ? seg < n_seg - 1 : seg < n_seg;
    int reduced = 0;
    float peak = 0.0f;
    double max_reduction = 0.0;
    if (mine) {
        const int len = eq_segment_len(n, seg);
        double* sp = state + (size_t)b * state_row + (size_t)seg;
        double e1 = PASS == 0 ? 0.0 : sp[0];
        double e = PASS == 2 ? sp[segs] : 0.0;
        float* t = cmp_tile + lane * EQ_LDS_STRIDE;
        if (PASS < 2) {
            if (len == EQ_SEG) {
#pragma unroll 8
                for (int i = 0; i < EQ_SEG; ++i) cmp_detect(k, (double)t[i], e1, e);
            } else {
                for (int i = 0; i < len; ++i) cmp_detect(k, (double)t[i], e1, e);
            }
            sp[PASS == 0 ? 0 : segs] = PASS == 0 ? e1 : e;
        } else {
            double* ep = envelope ? envelope + (size_t)b * row + (size_t)seg * EQ_SEG : nullptr;
            for (int i = 0; i < len; ++i) {
                const float xf = t[i];
                const double ev = cmp_detect(k, (double)xf, e1, e);
                if (ep) ep[i] = ev;
                const double r = cmp_reduction(k, 20.0 * log10(ev));
                const double z = r + k.makeup;
                float o = xf;
                if (z != 0.0) {
                    o = (float)((double)xf * pow(10.0, z / 20.0));
                    t[i] = o;
                }
                if (r < 0.0) {
                    ++reduced;
                    max_reduction = fmax(max_reduction, -r);
                }
                peak = fmaxf(peak, fabsf(o));   // (a NaN is passed over)
            }
        }
    }
    if (PASS == 2) {
        if (partial) {   // (uniform)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                reduced += __shfl_xor(reduced, d, 64);
                peak = fmaxf(peak, __shfl_xor(peak, d, 64));
                max_reduction = fmax(max_reduction, __shfl_xor(max_reduction, d, 64));
            }
            if (lane == 0) partial[(size_t)b * partial_row + blockIdx.x] = CmpPartial{reduced, peak, max_reduction};
        }
        __syncthreads();
        eq_move_tile<false>(out + (size_t)b * row, first, count, cmp_tile, lane);
    }
}

// In place: the end states of a pass become the segments' initial states.  One wave per utterance takes 64 end states a load (lane
// l the one of segment base + l), runs the 64 links in turn -- the value of link j comes from lane j -- and stores the 64 initial
// states at once.  WHICH 0: s' = max(c, mult s) on the front half of the row's states; 1: t' = mult t + q on the back half.
template <int WHICH>
__global__ __launch_bounds__(EQ_LANES) void cmp_chain_kernel(CmpLens lens, double mult, double* __restrict__ state, size_t state_row, size_t segs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long n_seg = eq_segments((long long)lens.n[b]);
    double* sp = state + (size_t)b * state_row + (WHICH ? segs : 0);
    double cur = 0.0;
    for (long long base = 0; base < n_seg; base += EQ_LANES) {
        const long long idx = base + lane;
        const double c = idx < n_seg - 1 ? sp[idx] : 0.0;
        const int links = (int)min((long long)EQ_LANES, n_seg - base);
        double own = 0.0;
        for (int j = 0; j < links; ++j) {
            if (lane == j) own = cur;
            const double cj = __shfl(c, j, 64);
            const double m = __dmul_rn(mult, cur);
            if (WHICH == 0)
                cur = cj > m ? cj : m;
            else
                cur = __dadd_rn(m, cj);
        }
        if (idx < n_seg) sp[idx] = own;
    }
}

// One wave per utterance: the record of a row out of its tiles' partials.
__global__ __launch_bounds__(EQ_LANES) void cmp_stats_kernel(CmpLens lens, const CmpPartial* __restrict__ partial, size_t partial_row,
                                                             tts_compress_stats_t* __restrict__ stats) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long n_tiles = eq_tiles((long long)lens.n[b]);
    int reduced = 0;
    float peak = 0.0f;
    double max_reduction = 0.0;
    for (long long i = lane; i < n_tiles; i += EQ_LANES) {
        const CmpPartial p = partial[(size_t)b * partial_row + (size_t)i];
        reduced += p.reduced;
        peak = fmaxf(peak, p.peak);
        max_reduction = fmax(max_reduction, p.max_reduction);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        reduced += __shfl_xor(reduced, d, 64);
        peak = fmaxf(peak, __shfl_xor(peak, d, 64));
        max_reduction = fmax(max_reduction, __shfl_xor(max_reduction, d, 64));
    }
    if (lane == 0) stats[b] = tts_compress_stats_t{lens.n[b], reduced, (float)max_reduction, peak};
}

}  // namespace tts

namespace tts_api {

// The workspaces of a tts_compress call on B rows of N samples; the partials only where records are asked for.
int compressor_scratch(tts_handle_t h, int B, int N, bool records, CmpScratch* s) {
    WS(h, "cmp.state", double, (size_t)B * cmp_state_doubles(N), state);
    *s = CmpScratch{state, nullptr};
    if (records) {
        WS(h, "cmp.partial", CmpPartial, (size_t)B * cmp_partials(N), partial);
        s->partial = partial;
    }
    return TTS_OK;
}

static CmpParams cmp_params_of(const tts_compressor_t& p) {
    return CmpParams{p.threshold_db, p.slope, p.knee_db, p.makeup_db, p.attack_coeff, p.release_coeff};
}

// On h->stream; everything has been checked (compressor_check).
int compressor_impl(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_compressor_t& params,
                    double* envelope, tts_compress_stats_t* stats) {
    CmpScratch s;
    const int rc = compressor_scratch(h, B, N, stats != nullptr, &s);
    if (rc) return rc;
    const CmpCoef k = cmp_coef(cmp_params_of(params));
    const size_t segs = (size_t)eq_segments(N), state_row = cmp_state_doubles(N), partial_row = cmp_partials(N);
    const size_t lds = eq_lds_bytes();   // (over 64 KB: asked for by name, as equalizer.hip does)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cmp_segments_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cmp_segments_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cmp_segments_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    HIPCHK(h, e);
    ProfScope ps(h, ST_COMPRESS, (int64_t)length_chunks(B, CMP_UTTS) * (stats ? 6 : 5));
    for (int b0 = 0; b0 < B; b0 += CMP_UTTS) {
        const int nb = std::min(CMP_UTTS, B - b0);
        CmpLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        const float* w = wav + (size_t)b0 * N;
        float* o = out + (size_t)b0 * N;
        double* st = s.state + (size_t)b0 * state_row;
        double* env = envelope ? envelope + (size_t)b0 * N : nullptr;
        CmpPartial* part = stats ? reinterpret_cast<CmpPartial*>(s.partial) + (size_t)b0 * partial_row : nullptr;
        const dim3 grid((unsigned)eq_tiles(longest), nb);
        hipLaunchKernelGGL(cmp_segments_kernel<0>, grid, dim3(EQ_LANES), lds, h->stream, w, o, (size_t)N, lens, k, st, state_row, segs, env, part, partial_row);
        hipLaunchKernelGGL(cmp_chain_kernel<0>, dim3(nb), dim3(EQ_LANES), 0, h->stream, lens, k.AR, st, state_row, segs);
        hipLaunchKernelGGL(cmp_segments_kernel<1>, grid, dim3(EQ_LANES), lds, h->stream, w, o, (size_t)N, lens, k, st, state_row, segs, env, part, partial_row);
        hipLaunchKernelGGL(cmp_chain_kernel<1>, dim3(nb), dim3(EQ_LANES), 0, h->stream, lens, k.AA, st, state_row, segs);
        hipLaunchKernelGGL(cmp_segments_kernel<2>, grid, dim3(EQ_LANES), lds, h->stream, w, o, (size_t)N, lens, k, st, state_row, segs, env, part, partial_row);
        if (stats) hipLaunchKernelGGL(cmp_stats_kernel, dim3(nb), dim3(EQ_LANES), 0, h->stream, lens, part, partial_row, stats + b0);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_compressor_design(int sampling_rate, double attack_ms, double release_ms, double* attack_coeff_out, double* release_coeff_out) {
    if (!attack_coeff_out || !release_coeff_out) return TTS_ERR_INVALID;
    double a = 0.0, r = 0.0;
    const std::string why = cmp_design(sampling_rate, attack_ms, release_ms, &a, &r);
    if (!why.empty()) return fail(nullptr, TTS_ERR_UNSUPPORTED, "compressor_design: " + why);
    *attack_coeff_out = a;
    *release_coeff_out = r;
    return TTS_OK;
}

int tts_compressor_profile(const char* name, int sampling_rate, tts_compressor_t* params_out) {
    bool invalid = false;
    CmpParams p{};
    const std::string why = cmp_profile(name, sampling_rate, params_out ? &p : nullptr, &invalid);
    if (!why.empty()) return fail(nullptr, invalid ? TTS_ERR_INVALID : TTS_ERR_UNSUPPORTED, "compressor_profile: " + why);
    *params_out = tts_compressor_t{p.threshold_db, p.slope, p.knee_db, p.makeup_db, p.attack_coeff, p.release_coeff};
    return TTS_OK;
}

int tts_compress(tts_handle_t h, const float* wav, float* out, int B, int N, const int32_t* n_samples, const tts_compressor_t* params,
                 double* envelope, tts_compress_stats_t* stats) {
    DeviceScope dev_scope(h);
    CmpParams p{};
    if (params) p = cmp_params_of(*params);
    const std::string why = compressor_check(reinterpret_cast<uintptr_t>(wav), reinterpret_cast<uintptr_t>(out), B, N, n_samples,
                                             params ? &p : nullptr, reinterpret_cast<uintptr_t>(envelope));
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "compress: " + why);
    if (!h) return TTS_ERR_INVALID;
    return compressor_impl(h, wav, out, B, N, n_samples, *params, envelope, stats);
}

int tts_set_compressor(tts_handle_t h, int enabled, const tts_compressor_t* params) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled) {
        const std::string why = params ? cmp_params_check(cmp_params_of(*params)) : std::string("a NULL pointer (params is required)");
        if (!why.empty()) return fail(h, TTS_ERR_INVALID, "set_compressor: " + why);
        h->settings.cmp.params = *params;
    }
    h->settings.cmp.enabled = enabled != 0;
    return TTS_OK;
}

}  // extern "C"
