// The join: pieces of the rows of a waveform batch laid one behind the other into output rows, with pauses or cross-fades between
// them (include/sstts_hip.h has the semantics, join_plan.h the layout and the cut).  A streaming copy with arithmetic at the edges
// of the pieces alone: 4 bytes read and 4 written per output sample, nothing kept.  The list travels by value, JOIN_PIECES pieces
// per launch; a launch writes the contiguous range of the flat output that its pieces own, so the launches of a call write every
// element once and none of them reads `out`.
#include "api_internal.h"
#include "join_plan.h"

namespace tts {

// one output sample that piece E owns, `rel` samples behind E's start; P: E's predecessor (read where rel < E.over)
__device__ __forceinline__ float join_sample(const float* __restrict__ wav, long long N, const JoinEntry& E, const JoinEntry& P, int fade, int rel) {
    if (rel >= E.count) return 0.f;   // the gap, or the rest of the row
    const float xb = wav[(long long)E.row * N + E.first + rel];
    const int f = join_fade(fade, E.count);
    if (rel < E.over) {   // (over <= f and over <= the predecessor's f: both samples are inside their fades)
        const int k = P.count - E.over + rel;
        const float xa = wav[(long long)P.row * N + P.first + k];
        const double a = (double)xa * join_gain(k, P.count, join_fade(fade, P.count));
        const double b = (double)xb * join_gain(rel, E.count, f);
        return (float)(a + b);
    }
    if (rel < f || rel >= E.count - f) return (float)((double)xb * join_gain(rel, E.count, f));
    return xb;
}

// Output samples [lo, hi) of the flat array out[G * N_out], owned by the pieces c.e[1 .. n] (c.e[q].start ascending, c.e[1].start ==
// lo).  The tiles are cut in u = flat index + mis, mis = the floats `out` lies behind a 16-byte boundary, so that a thread's four
// samples u0 .. u0 + 3 are one aligned store wherever all four are the launch's; a piece starts at any sample, so the four source
// floats of a thread lie at a 4-byte boundary: the compiler reads them with one global_load_dwordx4, which gfx950 takes at any
// dword address, and the per-sample path at the edges float by float.  tile0: the tile of lo + mis.
__global__ __launch_bounds__(JOIN_THREADS) void join_kernel(const float* __restrict__ wav, long long N, const JoinChunk c, int n, long long lo,
                                                            long long hi, int fade, int mis, long long tile0, float* __restrict__ out) {
    const long long t0 = (tile0 + blockIdx.x) * JOIN_TILE - mis;   // the tile's first flat index (may lie in front of lo)
    const long long t1 = t0 + JOIN_TILE;
    const long long e0 = t0 + 4 * (long long)threadIdx.x;
    // the first piece whose owned range ends behind the tile's start (workgroup-uniform; the range of piece q ends at the start of q + 1)
    int a = 1, b = n;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (c.e[m + 1].start > t0) b = m;
        else a = m + 1;
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int have = 0;
    for (int q = a; q <= n && c.e[q].start < t1; ++q) {
        const JoinEntry E = c.e[q], P = c.e[q - 1];
        const long long end = q < n ? c.e[q + 1].start : hi;
        const long long r0 = e0 - E.start;   // the thread's first sample, relative to the piece
        if (r0 + 3 < 0 || e0 >= end) continue;
        const int f = join_fade(fade, E.count);
        if (r0 >= f && r0 + 3 < (long long)E.count - f && e0 + 3 < end) {   // four samples of the piece's inside (over <= f)
            const float* s = wav + (long long)E.row * N + E.first + r0;
            v[0] = s[0], v[1] = s[1], v[2] = s[2], v[3] = s[3];
            have = 15;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long e = e0 + j;
            if (e >= E.start && e < end && e >= lo) {
                v[j] = join_sample(wav, N, E, P, fade, (int)(e - E.start));
                have |= 1 << j;
            }
        }
    }
    if (have == 15) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (have & (1 << j)) out[e0 + j] = v[j];
    }
}

}  // namespace tts

namespace tts_api {

// On h->stream; everything has been checked.  e: join_entries' P + 1 entries.
static int join_impl(tts_handle_t h, const float* wav, int N, const std::vector<JoinEntry>& e, int P, int G, int fade, int N_out, float* out) {
    const long long total = (long long)G * N_out;
    const int mis = (int)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
    ProfScope ps(h, ST_JOIN, join_launches(P));
    for (int p0 = 0; p0 < P; p0 += JOIN_PIECES) {
        const int n = std::min(JOIN_PIECES, P - p0);
        JoinChunk c;
        for (int q = 0; q <= JOIN_PIECES; ++q) c.e[q] = q <= n ? e[(size_t)p0 + q] : JoinEntry{0, 0, 0, 0, 0};
        const long long lo = c.e[1].start, hi = p0 + n < P ? e[(size_t)p0 + n + 1].start : total;
        const long long tile0 = (lo + mis) / JOIN_TILE, tile1 = (hi - 1 + mis) / JOIN_TILE;
        hipLaunchKernelGGL(join_kernel, dim3((unsigned)(tile1 - tile0 + 1)), dim3(JOIN_THREADS), 0, h->stream, wav, (long long)N, c, n, lo, hi, fade,
                           mis, tile0, out);
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_join_plan(const tts_join_piece_t* pieces, int P, const int32_t* group, int G, int B, int N, int fade, int64_t* n_out) {
    const std::string why = join_plan(pieces, P, group, G, B, N, fade, n_out);
    return why.empty() ? TTS_OK : fail(nullptr, TTS_ERR_INVALID, "join_plan: " + why);   // (no handle: tts_last_error(NULL) has the text)
}

int tts_join(tts_handle_t h, const float* wav, int B, int N, const tts_join_piece_t* pieces, int P, const int32_t* group, int G, int fade, int N_out,
             float* out) {
    DeviceScope dev_scope(h);
    std::string why;
    std::vector<int64_t> n_out, offset;
    if (!wav || !out) {
        why = "a NULL pointer (wav, pieces, group and out are required)";
    } else {
        n_out.resize(G > 0 && G <= JOIN_MAX_PIECES ? (size_t)G : 1);   // (join_plan refuses G > P before it writes a length)
        offset.resize(P > 0 && P <= JOIN_MAX_PIECES ? (size_t)P : 1);
        why = join_plan(pieces, P, group, G, B, N, fade, n_out.data(), offset.data());
        if (why.rfind("a NULL pointer", 0) == 0) why = "a NULL pointer (wav, pieces, group and out are required)";
    }
    if (why.empty()) why = join_room(n_out.data(), G, N_out);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out)) & 3)) why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "join: " + why);
    if (!h) return TTS_ERR_INVALID;
    std::vector<JoinEntry> e;
    join_entries(pieces, P, group, N_out, offset.data(), e);
    return join_impl(h, wav, N, e, P, G, fade, N_out, out);
}

int tts_join_max_pieces(void) { return JOIN_MAX_PIECES; }
int tts_join_max_fade(void) { return JOIN_MAX_FADE; }
int tts_join_tile(void) { return JOIN_TILE; }

}  // extern "C"
