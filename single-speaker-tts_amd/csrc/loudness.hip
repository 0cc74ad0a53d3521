// Loudness: integrated loudness after ITU-R BS.1770-4 / EBU R 128 of batches of mono waveforms (K-weighting, 400 ms blocks, the
// absolute and the relative gate) and the gain that takes an utterance to a target in LUFS under a peak ceiling.  No reference
// counterpart.  include/sstts_hip.h has the definition in full and loudness_plan.h the cut; every operation is an individually
// rounded IEEE double operation, so the results are the bits of tests/loudness_oracle.py.
//
// The K-weighting recurrence is sequential, so an utterance is cut into segments (8 per 100 ms step, loudness_plan.h) and a lane
// owns a segment:
//   loud_segments_kernel<false>  the cascade over the segment from the zero state; keeps the state it ends in
//   loud_chain_kernel            one wave per utterance chains those states with the segments' 4 x 4 transitions, 16 segments per
//                                round: the lanes load a round's 64 end-state values side by side, a quad of lanes owns the four
//                                rows of the chain, and lane 4 g + r keeps value r of the state in front of segment g
//   loud_segments_kernel<true>   the segment again from its initial state; the sum of y * y in sample order
//   loud_gate_kernel             a workgroup per utterance: the step sums, the block means, then one wave walks the blocks in
//                                order twice on broadcast values (the absolute gate's mean, then the relative gate's)
// A lane reads its segment in register tiles of 16 samples, the next tile in flight while this one runs; neighbouring lanes are a
// segment apart, so a wave touches 64 cache lines which it uses up over two tiles.  The passes are bound by the latency of the
// recurrence, not by memory.
// The normaliser adds the peak over the finite samples (an integer maximum of bit patterns: order-free), the gain and a scaling
// pass.  No floating-point atomics; every loop bound is a host value that travelled in the launch.
#include "api_internal.h"
#include "loudness_plan.h"

// y = b0 x + z1 is a product and a sum (tests/loudness_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

struct LoudLens {
    int n[LOUD_UTTS];
};

// what the kernels know of a sampling rate
struct LoudPlan {
    double k[10];     // the filters
    double Mc[16];    // the transition of a segment of c samples
    double Ml[16];    // ... of a step's last segment
    int sr;
};

constexpr int LOUD_LANES = 256;
constexpr int LOUD_SCALE_PER_LANE = 16;
constexpr int LOUD_TILE = 16;   // samples a lane holds in registers ahead of the recurrence

// the value of lane J of every quad, in all four of its lanes
template <int J>
__device__ __forceinline__ double loud_quad(double v) {
    constexpr int CTRL = J * 0x55;   // quad_perm [J, J, J, J]
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// wav points at the first utterance of the launch, row floats apart; ws at its workspace, ws_row doubles apart: the states
// [segments][4], behind them (sums_at) the segment sums.
template <bool SUM>
__global__ __launch_bounds__(LOUD_LANES) void loud_segments_kernel(const float* __restrict__ wav, size_t row, LoudLens lens, LoudPlan plan,
                                                                   double* __restrict__ ws, size_t ws_row, size_t sums_at) {
    const int b = blockIdx.y;
    const int K = loud_steps_read(lens.n[b], plan.sr);
    const long long g = (long long)blockIdx.x * LOUD_LANES + threadIdx.x;
    if (g >= (long long)K * LOUD_SEGS) return;
    const int s = loud_step(plan.sr), c = loud_segment(plan.sr);
    const int q = (int)(g % LOUD_SEGS);
    const int len = loud_segment_len(plan.sr, q);
    const float* x = wav + (size_t)b * row + (size_t)(g / LOUD_SEGS) * s + (size_t)q * c;   // (the segment ends inside K s <= n_b)
    double* state = ws + (size_t)b * ws_row + (size_t)g * 4;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (SUM) {
#pragma unroll
        for (int r = 0; r < 4; ++r) st[r] = state[r];
    }
    double acc = 0.0;
    // The samples come in register tiles, the next one loaded while this one runs, the last (partial) one ahead of them all: a
    // lane's reads are a segment apart from its neighbours', and the recurrence would otherwise wait for every one of them.
    const int full = len / LOUD_TILE;
    float cur[LOUD_TILE], nxt[LOUD_TILE], rest[LOUD_TILE];
#pragma unroll
    for (int j = 0; j < LOUD_TILE; ++j) {
        rest[j] = full * LOUD_TILE + j < len ? x[full * LOUD_TILE + j] : 0.f;
        cur[j] = j < len ? x[j] : 0.f;
        nxt[j] = 0.f;
    }
    for (int t = 0; t < full; ++t) {
        if (t + 1 < full) {
#pragma unroll
            for (int j = 0; j < LOUD_TILE; ++j) nxt[j] = x[(t + 1) * LOUD_TILE + j];
        }
#pragma unroll
        for (int j = 0; j < LOUD_TILE; ++j) {
            const double y = loud_sample(plan.k, st, (double)cur[j]);
            if (SUM) acc = __dadd_rn(acc, __dmul_rn(y, y));
        }
#pragma unroll
        for (int j = 0; j < LOUD_TILE; ++j) cur[j] = nxt[j];
    }
#pragma unroll
    for (int j = 0; j < LOUD_TILE; ++j) {
        if (full * LOUD_TILE + j < len) {
            const double y = loud_sample(plan.k, st, (double)rest[j]);
            if (SUM) acc = __dadd_rn(acc, __dmul_rn(y, y));
        }
    }
    if (SUM) {
        ws[(size_t)b * ws_row + sums_at + (size_t)g] = acc;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) state[r] = st[r];
    }
}

// In place: the end states of pass 1 become the segments' initial states.  One wave per utterance; a round is 16 segments = the
// 64 doubles the lanes load side by side.  Lane 4 g + r owns row r of the chain: it holds S[r], takes the other three values
// from its quad, and keeps the S[r] in front of segment g of the round.  The next round's end states are loaded while this
// round's links run.
__global__ __launch_bounds__(64) void loud_chain_kernel(LoudLens lens, LoudPlan plan, double* __restrict__ ws, size_t ws_row) {
    const int b = blockIdx.x, lane = threadIdx.x, r = lane & 3, slot = lane >> 2;
    const long long n_val = (long long)loud_steps_read(lens.n[b], plan.sr) * LOUD_SEGS * 4;   // doubles of state: a multiple of 32
    double* state = ws + (size_t)b * ws_row;
    double mc[4], ml[4];   // row r of the two transitions
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mc[j] = r == 0 ? plan.Mc[j] : r == 1 ? plan.Mc[4 + j] : r == 2 ? plan.Mc[8 + j] : plan.Mc[12 + j];
        ml[j] = r == 0 ? plan.Ml[j] : r == 1 ? plan.Ml[4 + j] : r == 2 ? plan.Ml[8 + j] : plan.Ml[12 + j];
    }
    double Sr = 0.0;
    double e_next = lane < n_val ? state[lane] : 0.0;
    for (long long v0 = 0; v0 < n_val; v0 += 64) {
        const double e = e_next;
        if (v0 + 64 + lane < n_val) e_next = state[v0 + 64 + lane];
        // (uniform; 16, or 8 in the last round: whole steps, and a round starts at a step's first segment)
        const int links = (int)min((long long)16, (n_val - v0) / 4);
        double mine = 0.0;
        for (int l0 = 0; l0 < links; l0 += LOUD_SEGS) {
#pragma unroll
            for (int q = 0; q < LOUD_SEGS; ++q) {
                const int l = l0 + q;
                const double el = __shfl(e, 4 * l + r, 64);   // e_l[r]
                if (l == slot) mine = Sr;
                const double S0 = loud_quad<0>(Sr), S1 = loud_quad<1>(Sr), S2 = loud_quad<2>(Sr), S3 = loud_quad<3>(Sr);
                const double* m = q == LOUD_SEGS - 1 ? ml : mc;
                Sr = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], S0), __dmul_rn(m[1], S1)), __dmul_rn(m[2], S2)), __dmul_rn(m[3], S3)), el);
            }
        }
        if (v0 + lane < n_val) state[v0 + lane] = mine;
    }
}

// sums, u and z: the utterance's segment sums, and room for its step sums and block means.  out: mean_square [B]; blocks: [B][2] or
// null.
__global__ __launch_bounds__(LOUD_LANES) void loud_gate_kernel(LoudLens lens, LoudPlan plan, double* __restrict__ ws, size_t ws_row, size_t sums_at,
                                                               size_t u_at, size_t z_at, double* __restrict__ out, int32_t* __restrict__ blocks) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = loud_steps_read(lens.n[b], plan.sr);
    const int J = K ? K - 3 : 0;
    const double* q = ws + (size_t)b * ws_row + sums_at;
    double* u = ws + (size_t)b * ws_row + u_at;
    double* z = ws + (size_t)b * ws_row + z_at;
    for (int k = tid; k < K; k += LOUD_LANES) {
        const double* p = q + (size_t)k * LOUD_SEGS;
        double a = __dadd_rn(p[0], p[1]);
#pragma unroll
        for (int i = 2; i < LOUD_SEGS; ++i) a = __dadd_rn(a, p[i]);
        u[k] = a;
    }
    __syncthreads();
    const double per_block = (double)(4 * loud_step(plan.sr));
    int bad = 0;
    for (int j = tid; j < J; j += LOUD_LANES) {
        const double v = __ddiv_rn(__dadd_rn(__dadd_rn(__dadd_rn(u[j], u[j + 1]), u[j + 2]), u[j + 3]), per_block);
        z[j] = v;
        bad |= !isfinite(v);
    }
    bad = __syncthreads_or(bad);   // (also: z is written)
    if (tid >= 64) return;
    double result = 0.0;
    int passed = 0;
    if (bad) {
        result = __builtin_nan("");   // a NaN or Inf sample in a counted block
    } else {
        // the absolute gate's mean, then the relative gate's: two walks in block order, every lane alike
        double threshold = LOUD_Z_ABS;
        for (int walk = 0; walk < 2; ++walk) {
            double sum = 0.0;
            int count = 0;
            for (int j0 = 0; j0 < J; j0 += 64) {
                const double mine = j0 + tid < J ? z[j0 + tid] : 0.0;
                const int n = min(64, J - j0);   // (uniform)
                for (int l = 0; l < n; ++l) {
                    const double v = __shfl(mine, l, 64);
                    if (v > LOUD_Z_ABS && v > threshold) {
                        sum = __dadd_rn(sum, v);
                        ++count;
                    }
                }
            }
            if (!count) break;   // no block passes: z = 0
            const double mean = __ddiv_rn(sum, (double)count);
            if (walk == 0) {
                threshold = __dmul_rn(LOUD_REL, mean);
            } else {
                result = mean;
                passed = count;
            }
        }
    }
    if (tid == 0) {
        out[b] = result;
        if (blocks) {
            blocks[2 * (size_t)b] = J;
            blocks[2 * (size_t)b + 1] = passed;
        }
    }
}

// peak[b] = the largest bit pattern of |x| over the finite samples (non-negative floats order as their bits); zeroed before.
__global__ __launch_bounds__(LOUD_LANES) void loud_peak_kernel(const float* __restrict__ wav, size_t row, LoudLens lens, unsigned* __restrict__ peak) {
    const int b = blockIdx.y;
    const int n = lens.n[b];
    const float* x = wav + (size_t)b * row;
    unsigned m = 0;
    const long long i0 = (long long)blockIdx.x * LOUD_LANES * LOUD_SCALE_PER_LANE + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < LOUD_SCALE_PER_LANE; ++j) {
        const long long i = i0 + (long long)j * LOUD_LANES;
        if (i < n) {
            const unsigned bits = __float_as_uint(x[i]) & 0x7fffffffu;
            if (bits < 0x7f800000u) m = max(m, bits);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(peak + b, m);
}

// gain[b] = min(sqrt(z_target / z), max_peak / peak); 1 where z is 0 or not finite or the peak is 0
__global__ void loud_gain_kernel(const double* __restrict__ z, const unsigned* __restrict__ peak, int nb, double z_target, double max_peak,
                                 double* __restrict__ gain, double* __restrict__ z_out, double* __restrict__ gain_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const double zb = z[b];
    const double pk = (double)__uint_as_float(peak[b]);
    double g = 1.0;
    if (isfinite(zb) && zb > 0.0 && pk > 0.0) {
        g = __dsqrt_rn(__ddiv_rn(z_target, zb));
        const double cap = __ddiv_rn(max_peak, pk);
        if (cap < g) g = cap;
    }
    gain[b] = g;
    if (z_out) z_out[b] = zb;
    if (gain_out) gain_out[b] = g;
}

__global__ __launch_bounds__(LOUD_LANES) void loud_scale_kernel(float* __restrict__ wav, size_t row, LoudLens lens, const double* __restrict__ gain) {
    const int b = blockIdx.y;
    const int n = lens.n[b];
    const double g = gain[b];
    float* x = wav + (size_t)b * row;
    const long long i0 = (long long)blockIdx.x * LOUD_LANES * LOUD_SCALE_PER_LANE + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < LOUD_SCALE_PER_LANE; ++j) {
        const long long i = i0 + (long long)j * LOUD_LANES;
        if (i < n) x[i] = (float)__dmul_rn(g, (double)x[i]);
    }
}

}  // namespace tts

namespace tts_api {

static LoudPlan loud_plan(int sr) {
    LoudPlan p;
    const LoudFilter f = loud_filter(sr);
    for (int i = 0; i < 10; ++i) p.k[i] = f.k[i];
    loud_transition(p.k, loud_segment(sr), p.Mc);
    loud_transition(p.k, loud_last_segment(sr), p.Ml);
    p.sr = sr;
    return p;
}

// The workspaces of a measurement of B rows of N samples.
int loudness_scratch(tts_handle_t h, int B, int N, int sr, LoudScratch* s) {
    WS(h, "loud.ws", double, (size_t)B * loud_ws_doubles(N, sr), ws);
    WS(h, "loud.z", double, (size_t)2 * B, zg);
    WS(h, "loud.peak", unsigned, (size_t)B, pk);
    *s = LoudScratch{ws, zg, pk};
    return TTS_OK;
}

// On h->stream; everything has been checked (loudness_check).  normalize: wav is scaled in place, mean_square and gain may be null.
int loudness_impl(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, int sr, bool normalize, double target_lufs, double max_peak,
                  double* mean_square, int32_t* n_blocks, double* gain) {
    const size_t ws_row = loud_ws_doubles(N, sr);
    LoudScratch s;
    const int rc = loudness_scratch(h, B, N, sr, &s);
    if (rc) return rc;
    const LoudPlan plan = loud_plan(sr);
    const size_t K = (size_t)loud_steps_read(N, sr);
    const size_t sums_at = K * LOUD_SEGS * 4, u_at = sums_at + K * LOUD_SEGS, z_at = u_at + K;
    const double z_target = normalize ? std::pow(10.0, (target_lufs + 0.691) / 10.0) : 0.0;
    ProfScope ps(h, ST_LOUDNESS, (int64_t)length_chunks(B, LOUD_UTTS) * (normalize ? 7 : 4) + (normalize ? 1 : 0));
    if (normalize) HIPCHK(h, hipMemsetAsync(s.peak, 0, (size_t)B * sizeof(unsigned), h->stream));
    for (int b0 = 0; b0 < B; b0 += LOUD_UTTS) {
        const int nb = std::min(LOUD_UTTS, B - b0);
        LoudLens lens;
        const int longest = fill_lengths(lens.n, n_samples, b0, nb, N);
        float* pw = wav + (size_t)b0 * N;
        double* pws = s.ws + (size_t)b0 * ws_row;
        double* pz = mean_square && !normalize ? mean_square + b0 : s.z + b0;
        const long long n_seg = (long long)loud_steps_read(longest, sr) * LOUD_SEGS;
        if (n_seg) {
            const dim3 grid((unsigned)((n_seg + LOUD_LANES - 1) / LOUD_LANES), nb);
            hipLaunchKernelGGL(loud_segments_kernel<false>, grid, dim3(LOUD_LANES), 0, h->stream, pw, (size_t)N, lens, plan, pws, ws_row, sums_at);
            hipLaunchKernelGGL(loud_chain_kernel, dim3(nb), dim3(64), 0, h->stream, lens, plan, pws, ws_row);
            hipLaunchKernelGGL(loud_segments_kernel<true>, grid, dim3(LOUD_LANES), 0, h->stream, pw, (size_t)N, lens, plan, pws, ws_row, sums_at);
        }
        hipLaunchKernelGGL(loud_gate_kernel, dim3(nb), dim3(LOUD_LANES), 0, h->stream, lens, plan, pws, ws_row, sums_at, u_at, z_at, pz,
                           n_blocks ? n_blocks + 2 * (size_t)b0 : nullptr);
        if (normalize) {
            const long long per_block = (long long)LOUD_LANES * LOUD_SCALE_PER_LANE;
            const dim3 grid((unsigned)((longest + per_block - 1) / per_block), nb);
            hipLaunchKernelGGL(loud_peak_kernel, grid, dim3(LOUD_LANES), 0, h->stream, pw, (size_t)N, lens, s.peak + b0);
            hipLaunchKernelGGL(loud_gain_kernel, dim3(1), dim3(LOUD_UTTS), 0, h->stream, pz, s.peak + b0, nb, z_target, max_peak, s.z + B + b0,
                               mean_square ? mean_square + b0 : nullptr, gain ? gain + b0 : nullptr);
            hipLaunchKernelGGL(loud_scale_kernel, grid, dim3(LOUD_LANES), 0, h->stream, pw, (size_t)N, lens, s.z + B + b0);
        }
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_loudness_filter(int sampling_rate, double coeffs[10]) {
    if (!coeffs) return TTS_ERR_INVALID;
    if (sampling_rate < LOUD_SR_MIN || sampling_rate > LOUD_SR_MAX) return TTS_ERR_UNSUPPORTED;
    const LoudFilter f = loud_filter(sampling_rate);
    for (int i = 0; i < 10; ++i) coeffs[i] = f.k[i];
    return TTS_OK;
}

int tts_loudness_segment(int sampling_rate) {
    return (sampling_rate < LOUD_SR_MIN || sampling_rate > LOUD_SR_MAX) ? 0 : loud_segment(sampling_rate);
}

int tts_loudness(tts_handle_t h, const float* wav, int B, int N, const int32_t* n_samples, int sampling_rate, double* mean_square,
                 int32_t* n_blocks) {
    DeviceScope dev_scope(h);
    bool unsupported = false;
    std::string why = loudness_check(wav && mean_square, B, N, n_samples, sampling_rate, false, 0.0, 1.0, &unsupported);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(mean_square) & 7) || ((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(n_blocks)) & 3)))
        why = "mean_square must be 8-byte aligned, the other buffers 4-byte aligned";
    if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "loudness: " + why);
    if (!h) return TTS_ERR_INVALID;
    return loudness_impl(h, const_cast<float*>(wav), B, N, n_samples, sampling_rate, false, 0.0, 1.0, mean_square, n_blocks, nullptr);
}

int tts_loudness_normalize(tts_handle_t h, float* wav, int B, int N, const int32_t* n_samples, int sampling_rate, double target_lufs,
                           double max_peak, double* mean_square, double* gain) {
    DeviceScope dev_scope(h);
    bool unsupported = false;
    std::string why = loudness_check(wav != nullptr, B, N, n_samples, sampling_rate, true, target_lufs, max_peak, &unsupported);
    if (why.empty() && (((reinterpret_cast<uintptr_t>(mean_square) | reinterpret_cast<uintptr_t>(gain)) & 7) || (reinterpret_cast<uintptr_t>(wav) & 3)))
        why = "mean_square and gain must be 8-byte aligned, wav 4-byte aligned";
    if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "loudness_normalize: " + why);
    if (!h) return TTS_ERR_INVALID;
    return loudness_impl(h, wav, B, N, n_samples, sampling_rate, true, target_lufs, max_peak, mean_square, nullptr, gain);
}

int tts_set_loudness(tts_handle_t h, int enabled, double target_lufs, double max_peak, int sampling_rate) {
    if (!h) return TTS_ERR_INVALID;
    if (enabled) {
        bool unsupported = false;
        const std::string why = loudness_check(true, 1, 1, nullptr, sampling_rate, true, target_lufs, max_peak, &unsupported);
        if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "set_loudness: " + why);
        h->settings.loud.target_lufs = target_lufs;
        h->settings.loud.max_peak = max_peak;
        h->settings.loud.sampling_rate = sampling_rate;
    }
    h->settings.loud.enabled = enabled != 0;
    return TTS_OK;
}

}  // extern "C"
