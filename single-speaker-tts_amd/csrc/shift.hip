// Formant-preserving pitch: a per-frame shift of magnitude spectrograms along the FREQUENCY axis, ahead of Griffin-Lim
// (include/sstts_hip.h has the semantics, shift_plan.h the cut and the LDS layout).  A frame x[0 .. N] is split into a smooth
// envelope -- the first Q cepstral coefficients of log x under a raised-cosine lifter -- and the fine structure x exp(-E); the fine
// structure is read at k * pitch_step / 65536, the envelope at k * formant_step / 65536, and the two are multiplied back.  All of
// it in double: the stage is held to tests/shift_oracle.py within 2^-24 |y| + eta (|t1| + |t2|), eta far below float32.
//
// A compute workgroup takes SHIFT_TILE consecutive frames of one segment, shift_pass_frames(N) at a time, in four phases:
//   1  x[k][t] from HBM (32-byte runs along T) into xs[t][k] (float) and L[t][k] = log(max(x, 1e-10)) (double); a frame with a
//      NaN or an Inf is flagged
//   2  c[t][q] = (1/N) sum_k w[k] L[t][k] ct[q k mod 2N]: eight lanes share a sum, lane p the bins 8 j + p with j ascending, then
//      a butterfly over the eight; hc[q][t] = h[q] c[t][q]
//   3  E[t][k] = sum_q hc[q][t] ct[q k mod 2N], q ascending, a thread per bin and all frames of the pass at once (one table read
//      feeds eight FMAs); E overwrites L
//   4  out[k][t] = exp(Ew) ((1 - a) X[i] + a X[i + 1]) with X[i] = xs[i] exp(-E[i]), stored in 32-byte runs along T
// The order of every sum depends on N and Q alone: a frame's bits do not depend on its tile, its segment, the launch or the batch.
// Copy tiles (uncovered frames, segments at 65536 / 65536, the rest of a row) move 4-byte words, 64 frames x all bins a workgroup.
#include "api_internal.h"
#include "shift_plan.h"

namespace tts {

__device__ __forceinline__ double shift_group_sum(double s) {   // over the SHIFT_PARTS = 8 adjacent lanes of a sum: the same bits in each
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    return s;
}

// SUB: shift_pass_frames(N), 8 or 4
template <int SUB>
__device__ __forceinline__ void shift_pass(const float* __restrict__ in, float* __restrict__ out, const double* __restrict__ ct_g,
                                           const double* __restrict__ h_g, size_t base, int t0, int nt, int N, int Q, int T, uint32_t pitch_step,
                                           uint32_t formant_step, double* ct, double* LE, double* hc, float* xs, int* bad, bool first_pass) {
    const int tid = threadIdx.x;
    const int F = N + 1, row = shift_row(N), mask = 2 * N - 1;
    if (first_pass)
        for (int j = tid; j < shift_ct_doubles(N); j += SHIFT_THREADS) ct[j] = ct_g[j];
    if (tid < SHIFT_TILE) bad[tid] = 0;
    __syncthreads();
    // ---- 1: load, log
    for (int id = tid; id < SUB * F; id += SHIFT_THREADS) {
        const int t = id & (SUB - 1), k = id / SUB;
        float x = 0.f;
        if (t < nt) {
            x = in[base + (size_t)k * T + (t0 + t)];
            if (!(fabsf(x) <= 3.402823466e38f)) bad[t] = 1;   // (NaN or Inf: every writer stores the same word)
        }
        const double xd = (double)x;
        xs[t * row + k] = x;
        LE[t * row + k] = xd != xd ? xd : log(xd > 1e-10 ? xd : 1e-10);
    }
    __syncthreads();
    // ---- 2: the cepstral coefficients, under the lifter
    const double inv_n = 1.0 / (double)N;
    for (int id0 = 0; id0 < SHIFT_PARTS * SUB * Q; id0 += SHIFT_THREADS) {   // (whole groups of eight lanes: SHIFT_THREADS is a multiple of 8)
        const int id = id0 + tid;
        const int p = id & (SHIFT_PARTS - 1), t = (id / SHIFT_PARTS) & (SUB - 1), qq = id / (SHIFT_PARTS * SUB);
        const int q = qq < Q ? qq : Q - 1;
        const double* Lt = LE + t * row;
        double s = 0.0;
        for (int k = p; k < N; k += SHIFT_PARTS) {
            const double l = k == 0 ? 0.5 * Lt[0] : Lt[k];
            s = fma(l, ct[shift_ct_slot((q * k) & mask)], s);
        }
        if (p == 0) s = fma(0.5 * Lt[N], ct[shift_ct_slot((q * N) & mask)], s);
        s = shift_group_sum(s);
        if (p == 0 && qq < Q) hc[q * SUB + t] = h_g[q] * (s * inv_n);
    }
    __syncthreads();
    // ---- 3: the envelope, over L
    for (int k = tid; k < F; k += SHIFT_THREADS) {
        double acc[SUB];
#pragma unroll
        for (int t = 0; t < SUB; ++t) acc[t] = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double c = ct[shift_ct_slot((q * k) & mask)];
#pragma unroll
            for (int t = 0; t < SUB; ++t) acc[t] = fma(hc[q * SUB + t], c, acc[t]);
        }
#pragma unroll
        for (int t = 0; t < SUB; ++t) LE[t * row + k] = acc[t];
    }
    __syncthreads();
    // ---- 4: move the fine structure and the envelope, multiply back
    const long long nyq = (long long)N << 16;
    for (int id = tid; id < SUB * F; id += SHIFT_THREADS) {
        const int t = id & (SUB - 1), k = id / SUB;
        if (t >= nt) continue;
        const double* Et = LE + t * row;
        const float* xt = xs + t * row;
        long long p = (long long)k * (long long)pitch_step;
        if (p > nyq) p = 2 * nyq - p;
        const int i = (int)(p >> 16), i1 = i + 1 < N ? i + 1 : N;
        const double a = (double)(p & 65535) * (1.0 / 65536.0);
        long long pf = (long long)k * (long long)formant_step;
        if (pf > nyq) pf = nyq;
        const int j = (int)(pf >> 16), j1 = j + 1 < N ? j + 1 : N;
        const double af = (double)(pf & 65535) * (1.0 / 65536.0);
        const double X0 = (double)xt[i] * exp(-Et[i]), X1 = (double)xt[i1] * exp(-Et[i1]);
        const double Xs = (1.0 - a) * X0 + a * X1;
        const double Ew = (1.0 - af) * Et[j] + af * Et[j1];
        float y = (float)(exp(Ew) * Xs);
        if (bad[t]) y = __int_as_float(0x7fc00000);
        out[base + (size_t)k * T + (t0 + t)] = y;
    }
    __syncthreads();   // (the next pass overwrites xs, LE and bad)
}

// mag [B][F][T] -> out [B][F][T].  blockIdx.x is the tile in the launch's numbering (segment_find).
__global__ __launch_bounds__(SHIFT_THREADS) void shift_kernel(const float* __restrict__ in, float* __restrict__ out, const ShiftChunk c, int n_seg,
                                                              int N, int Q, int T, const double* __restrict__ ct_g, const double* __restrict__ h_g) {
    extern __shared__ __align__(16) double shift_lds[];
    const int tile = blockIdx.x;
    const ShiftEntry E = c.e[segment_find(c.e, n_seg, tile)];
    const ShiftTile w = shift_tile_of(E, tile - E.tile0);
    const int F = N + 1;
    const size_t base = (size_t)E.row * F * T;
    if (!w.compute) {   // words: a wave per bin, its lanes along the frames; frames at or behind the row's length are +0.0 and never read
        const int t = w.t0 + (threadIdx.x & 63);
        if (t >= w.t1) return;
        const unsigned* src = reinterpret_cast<const unsigned*>(in) + base + t;
        unsigned* dst = reinterpret_cast<unsigned*>(out) + base + t;
        const bool live = t < E.n;
        for (int k = threadIdx.x >> 6; k < F; k += SHIFT_THREADS / 64) dst[(size_t)k * T] = live ? src[(size_t)k * T] : 0u;
        return;
    }
    const int sub = shift_pass_frames(N);
    double* ct = shift_lds;
    double* LE = ct + shift_ct_doubles(N);
    double* hc = LE + sub * shift_row(N);
    float* xs = reinterpret_cast<float*>(hc + Q * sub);
    int* bad = reinterpret_cast<int*>(xs + sub * shift_row(N));
    for (int t0 = w.t0; t0 < w.t1; t0 += sub) {
        const int nt = min(sub, w.t1 - t0);
        if (sub == 8) shift_pass<8>(in, out, ct_g, h_g, base, t0, nt, N, Q, T, E.pitch_step, E.formant_step, ct, LE, hc, xs, bad, t0 == w.t0);
        else shift_pass<4>(in, out, ct_g, h_g, base, t0, nt, N, Q, T, E.pitch_step, E.formant_step, ct, LE, hc, xs, bad, t0 == w.t0);
    }
}

}  // namespace tts

namespace tts_api {

// The tables on the device: ct per N (padded: shift_ct_slot) and the lifter per Q.  Built on the host in double at the first call
// that asks for them, uploaded with a synchronous copy and kept by the handle.
static int shift_upload(tts_handle_t h, const std::vector<double>& host, double** out) {
    double* dev = nullptr;
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&dev), host.size() * sizeof(double)));
    const hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(dev);
        HIPCHK(h, e);
    }
    *out = dev;
    return TTS_OK;
}

static int shift_tables(tts_handle_t h, int N, int Q, const double** ct, const double** lifter) {
    auto it = h->shift.ct.find(N);
    if (it == h->shift.ct.end()) {
        if (!h->shift.configured) {
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&shift_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SHIFT_LDS_LIMIT));
            h->shift.configured = true;
        }
        double* dev = nullptr;
        const int rc = shift_upload(h, shift_cos_table_padded(N), &dev);
        if (rc != TTS_OK) return rc;
        it = h->shift.ct.emplace(N, dev).first;
    }
    auto il = h->shift.lifter.find(Q);
    if (il == h->shift.lifter.end()) {
        double* dev = nullptr;
        const int rc = shift_upload(h, shift_lifter(Q), &dev);
        if (rc != TTS_OK) return rc;
        il = h->shift.lifter.emplace(Q, dev).first;
    }
    *ct = it->second;
    *lifter = il->second;
    return TTS_OK;
}

void shift_release(tts_handle_t h) {
    for (auto& kv : h->shift.ct) hipFree(kv.second);
    for (auto& kv : h->shift.lifter) hipFree(kv.second);
    h->shift.ct.clear();
    h->shift.lifter.clear();
}

// On h->stream; everything has been checked.  e, tiles: shift_entries' S entries and the tiles of every launch.
static int shift_impl(tts_handle_t h, const float* mag, int N, int T, const std::vector<ShiftEntry>& e, const std::vector<int64_t>& tiles, int Q, float* out) {
    const double *ct = nullptr, *lifter = nullptr;
    const int rc = shift_tables(h, N, Q, &ct, &lifter);
    if (rc != TTS_OK) return rc;
    ProfScope ps(h, ST_SHIFT, (int64_t)tiles.size());
    const size_t lds = shift_lds_bytes(N, Q);
    return for_each_segment_launch(e, SHIFT_NO_ENTRY, [&](const ShiftChunk& c, int n, int l) -> int {
        hipLaunchKernelGGL(shift_kernel, dim3((unsigned)tiles[(size_t)l]), dim3(SHIFT_THREADS), lds, h->stream, mag, out, c, n, N, Q, T, ct, lifter);
        HIPCHK(h, hipGetLastError());
        return TTS_OK;
    });
}

}  // namespace tts_api

extern "C" {

int tts_shift_plan(const tts_shift_segment_t* segments, int S, int B, int F, int T, const int32_t* n_frames, int order) {
    const std::string why = shift_plan(segments, S, B, F, T, n_frames, order);
    return why.empty() ? TTS_OK : fail(nullptr, TTS_ERR_INVALID, "shift_plan: " + why);   // (no handle: tts_last_error(NULL) has the text)
}

int tts_shift_magnitudes(tts_handle_t h, const float* mag, int B, int F, int T, const int32_t* n_frames, const tts_shift_segment_t* segments, int S,
                         int order, float* out) {
    DeviceScope dev_scope(h);
    std::string why;
    if (!mag || !out || !segments) why = "a NULL pointer (mag, segments and out are required)";
    else if (out == mag) why = "out is mag: the stage does not work in place";
    else why = shift_plan(segments, S, B, F, T, n_frames, order);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(mag) | reinterpret_cast<uintptr_t>(out)) & 3)) why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "shift_magnitudes: " + why);
    if (!h) return TTS_ERR_INVALID;
    std::vector<ShiftEntry> e;
    std::vector<int64_t> tiles;
    shift_entries(segments, S, T, n_frames, e, tiles);
    return shift_impl(h, mag, F - 1, T, e, tiles, order, out);
}

int tts_shift_max_segments(void) { return SHIFT_MAX_SEGMENTS; }
int tts_shift_tile(void) { return SHIFT_TILE; }
int tts_shift_max_order(void) { return SHIFT_MAX_ORDER; }

}  // extern "C"
