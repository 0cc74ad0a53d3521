// Prosody: a segment-wise warp of magnitude spectrograms ahead of Griffin-Lim (include/sstts_hip.h has the semantics, warp_plan.h
// the layout and the cut).  The uniform stretch of stretch.hip with a piecewise-linear time map instead of k * rate: output frame
// o + j of a speech segment is the blend of the source frames i and i + 1 at
//   p = j * step;   i = first + (p >> 16), a = (p & 65535) * 2^-16;   y = (float)(g * ((1 - a) x[i] + a x[i + 1]))
// in double, every operation rounded on its own (no FMA), one rounding to float32; frame i + 1 at or behind the row's n_frames
// reads as 0.0 and is never fetched; a pause and the rest of a row are +0.0.  One HBM-bound pass in the reference's (F, T) layout:
// at most two source frames read and one written per output frame.  The list travels by value, WARP_SEGMENTS segments per launch:
// nothing is uploaded and nothing synchronised.  No atomics; a row's output does not depend on the batch it is in.
#include "api_internal.h"
#include "warp_plan.h"

// No contraction anywhere in this file: g * ((1 - a) x0 + a x1) is three products and a sum.  The compiler fuses through
// __dmul_rn / __dadd_rn too, so the file is also built with -ffp-contract=off (build.py).
#pragma clang fp contract(off)

namespace tts {

// mag [B][F][T] -> out [B][F][T_out]; the parent is stretch_cols_kernel: threads along the output frames, so the stores are
// contiguous along T, and the loads of a wave gather along the contiguous axis at stride `step` (0.25 .. 4 floats), two
// neighbours per output, inside the few cache lines its 64 outputs span: no staging.  Here a workgroup takes one tile of one
// segment -- blockIdx.x is the tile in the launch's numbering (segment_find) -- in the bins blockIdx.y * WARP_BINS ..: a thread
// computes i and a of its frame once and then walks the bins, wave w of the workgroup the bins w, w + 4, ...
__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(const float* __restrict__ in, float* __restrict__ out, const WarpChunk c, int n_seg, int F,
                                                            int T, int T_out) {
    const int tile = blockIdx.x;
    const WarpEntry E = c.e[segment_find(c.e, n_seg, tile)];
    const int j = (tile - E.tile0) * WARP_TILE + (threadIdx.x & (WARP_TILE - 1));
    if (j >= E.span) return;   // (behind what the segment owns: the next tile is the next segment's)
    const bool live = j < E.count;
    const long long p = (long long)j * (long long)E.step;
    const int i = live ? E.first + (int)(p >> 16) : 0;   // (live: i < first + frames <= n)
    const bool h1 = live && i + 1 < E.n;                 // (beyond: reads as 0.0, never fetched)
    const double a = (double)(p & 65535) * (1.0 / 65536.0), w0 = __dsub_rn(1.0, a), g = (double)E.gain;
    const float* src = in + (size_t)E.row * F * T + i;
    float* dst = out + (size_t)E.row * F * T_out + E.o + j;
    for (int f0 = blockIdx.y * WARP_BINS; f0 < F; f0 += gridDim.y * WARP_BINS) {   // (one round unless F > 65535 * WARP_BINS)
        const int f1 = min(F, f0 + WARP_BINS);
#pragma unroll 4
        for (int f = f0 + (threadIdx.x / WARP_TILE); f < f1; f += WARP_THREADS / WARP_TILE) {
            float y = 0.f;
            if (live) {
                const float x0 = src[(size_t)f * T];
                const float x1 = h1 ? src[(size_t)f * T + 1] : 0.f;
                y = (float)__dmul_rn(g, __dadd_rn(__dmul_rn(w0, (double)x0), __dmul_rn(a, (double)x1)));
            }
            dst[(size_t)f * T_out] = y;
        }
    }
}

}  // namespace tts

namespace tts_api {

// On h->stream; everything has been checked.  e, tiles: warp_entries' S entries and the tiles of every launch.
static int warp_impl(tts_handle_t h, const float* mag, int F, int T, const std::vector<WarpEntry>& e, const std::vector<int64_t>& tiles, int T_out,
                     float* out) {
    ProfScope ps(h, ST_WARP, (int64_t)tiles.size());
    const unsigned bins = (unsigned)std::min((F + WARP_BINS - 1) / WARP_BINS, 65535);
    return for_each_segment_launch(e, WARP_NO_ENTRY, [&](const WarpChunk& c, int n, int l) -> int {
        hipLaunchKernelGGL(warp_kernel, dim3((unsigned)tiles[(size_t)l], bins), dim3(WARP_THREADS), 0, h->stream, mag, out, c, n, F, T, T_out);
        HIPCHK(h, hipGetLastError());
        return TTS_OK;
    });
}

}  // namespace tts_api

extern "C" {

int tts_warp_plan(const tts_warp_segment_t* segments, int S, int B, int T, const int32_t* n_frames, int64_t* n_out) {
    const std::string why = warp_plan(segments, S, B, T, n_frames, n_out);
    return why.empty() ? TTS_OK : fail(nullptr, TTS_ERR_INVALID, "warp_plan: " + why);   // (no handle: tts_last_error(NULL) has the text)
}

int tts_warp_magnitudes(tts_handle_t h, const float* mag, int B, int F, int T, const int32_t* n_frames, const tts_warp_segment_t* segments, int S,
                        int T_out, float* out) {
    DeviceScope dev_scope(h);
    std::string why;
    std::vector<int64_t> n_out, count;
    if (!mag || !out || !segments) {
        why = "a NULL pointer (mag, segments and out are required)";
    } else if (F < 1) {
        why = "need B, F, T, S >= 1";
    } else {
        n_out.resize(B > 0 && B <= WARP_MAX_SEGMENTS ? (size_t)B : 1);   // (warp_plan refuses B > S before it reads or writes a length)
        count.resize(S > 0 && S <= WARP_MAX_SEGMENTS ? (size_t)S : 1);
        why = warp_plan(segments, S, B, T, n_frames, n_out.data(), count.data());
        if (why == "need B, T, S >= 1") why = "need B, F, T, S >= 1";
    }
    if (why.empty()) why = warp_room(n_out.data(), B, T_out);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(mag) | reinterpret_cast<uintptr_t>(out)) & 3)) why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "warp_magnitudes: " + why);
    if (!h) return TTS_ERR_INVALID;
    std::vector<WarpEntry> e;
    std::vector<int64_t> tiles;
    warp_entries(segments, S, T, n_frames, T_out, count.data(), e, tiles);
    return warp_impl(h, mag, F, T, e, tiles, T_out, out);
}

int tts_warp_max_segments(void) { return WARP_MAX_SEGMENTS; }
int tts_warp_tile(void) { return WARP_TILE; }

}  // extern "C"
