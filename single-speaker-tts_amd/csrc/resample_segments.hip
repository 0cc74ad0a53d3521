// Per-word pitch: a segment-wise resampler behind Griffin-Lim (include/sstts_hip.h has the semantics, resample_segments_plan.h the
// layout and the cut).  tts_resample with a ratio that changes along the row: output sample o + j of a segment at ratio rho != 1 is
// resample.hip's sum with the position measured from the segment's first sample,
//   tr = j / rho, m = first + (int)tr, frac = scale (tr - (int)tr);   f = 512 frac, off = (int)f, eta = f - off
//   y  = sum_i (win[off + i step] + eta delta[off + i step]) x[m - i]            i < (32769 - off) / step
//      + the same with frac = scale - frac on x[m + 1 + k]                        k < (32769 - off) / step
// in double, rounded once to float32, with x the ROW's samples: the taps reach over the segment's borders, and a sample outside
// [0, n_samples[row]) is 0.0 and never fetched (a product with 0.0 leaves a sum's bits alone, so the wings need no cut at the row's
// ends).  A segment at ratio 1.0 exactly is a copy: its floats are moved, bit for bit.  The index arithmetic is rounded operation
// by operation (no contraction: the file is built with -ffp-contract=off); the weights and the sum use explicit FMAs.
//
// warp.hip's scheme: the list travels by value, RSEG_SEGMENTS segments per launch; a workgroup takes one tile of RSEG_TILE
// consecutive output samples of one segment -- blockIdx.x is the tile in the launch's numbering (segment_find).  resample_kernel<1>'s
// tile: the samples the windows of the tile's outputs cover are staged in LDS, zero-filled outside the row, and one thread per
// output walks its two wings over its ratio's phase-major table (resample_plan.h), read out of L2.  Every row carries its own
// ratios, so a weight serves one sample, not the RS_U = 8 of the batched resampler.  No atomics; a row's output does not depend on
// the batch it is in nor on where its segments fall among the launches.
#include "api_internal.h"
#include "resample_segments_plan.h"

#pragma clang fp contract(off)

namespace tts {

constexpr int RSEG_TABLES = RSEG_MAX_RATIOS + 1;   // the ratios below 1 of a call, and in front of them the table of those above

struct RsegTables {
    const double2* t[RSEG_TABLES];
};

// one wing into the output's accumulator: tap i is an FMA of its weight, fma(eta, delta, win), and the sample i steps along `dir`
__device__ __forceinline__ double rseg_wing(const double2* __restrict__ trow, int cnt, double eta, const float* xp, int dir, double acc) {
#pragma unroll 8
    for (int i = 0; i < cnt; ++i) {
        const double2 wd = trow[i];
        acc = fma(fma(eta, wd.y, wd.x), (double)xp[(ptrdiff_t)dir * i], acc);
    }
    return acc;
}

// x [B][n] -> out [B][N_out] for the n_seg segments of the launch's chunk; lds_floats: the dynamic LDS of the launch
__global__ __launch_bounds__(RSEG_TILE) void resample_segments_kernel(const float* __restrict__ x, float* __restrict__ out, const RsegChunk c,
                                                                      const RsegTables tabs, int n_seg, int n, int N_out, int lds_floats) {
    extern __shared__ __align__(16) float rseg_xs[];
    const int tile = blockIdx.x;
    const RsegEntry E = c.e[segment_find(c.e, n_seg, tile)];
    const int j0 = (tile - E.tile0) * RSEG_TILE;
    const int j = j0 + (int)threadIdx.x;
    const float* src = x + (size_t)E.row * n;
    float* dst = out + (size_t)E.row * N_out + E.o;
    if (E.tab < 0) {   // a copy (and the zeros behind a row's last one): the floats are moved as they are
        if (j < E.span) {
            uint32_t v = 0u;
            if (j < E.count) v = reinterpret_cast<const uint32_t*>(src)[E.first + j];
            reinterpret_cast<uint32_t*>(dst)[j] = v;
        }
        return;
    }
    double acc = 0.0;
    if (j0 < E.count) {   // (uniform over the workgroup; otherwise the tile is zeros only)
        const int step = (int)(E.scale * (double)RS_NUM_TABLE);
        const int taps_max = RS_NWIN / step, row = (taps_max + 7) / 8 * 8;
        const double2* __restrict__ tab = tabs.t[E.tab];
        const int j_last = min(j0 + RSEG_TILE - 1, E.count - 1);
        const long long m_first = (long long)((double)j0 * E.inc), m_last = (long long)((double)j_last * E.inc);
        const long long lo = (long long)E.first + m_first - (taps_max - 1);
        const int staged = min((int)(m_last - m_first) + 2 * taps_max, lds_floats);   // (never cut: rseg_span_max; a guard for the LDS stores)
        for (int idx = threadIdx.x; idx < staged; idx += RSEG_TILE) {
            const long long g = lo + idx;
            rseg_xs[idx] = (g >= 0 && g < E.n) ? src[g] : 0.f;
        }
        __syncthreads();
        if (j <= j_last) {
            const double tr = (double)j * E.inc;
            const long long m = (long long)tr;
            double frac = E.scale * (tr - (double)m);
            const int at = (int)(m - m_first) + taps_max - 1;   // first + m in the staged samples: taps_max - 1 <= at, at + taps_max < staged
            {
                const double f = frac * (double)RS_NUM_TABLE;
                const int off = (int)f;
                const double eta = f - (double)off;
                acc = rseg_wing(tab + (size_t)off * row, (RS_NWIN - off) / step, eta, rseg_xs + at, -1, acc);
            }
            {   // (the right wing goes on where the left one ended: one accumulator)
                frac = E.scale - frac;
                const double f = frac * (double)RS_NUM_TABLE;
                const int off = (int)f;
                const double eta = f - (double)off;
                acc = rseg_wing(tab + (size_t)off * row, (RS_NWIN - off) / step, eta, rseg_xs + at + 1, 1, acc);
            }
        }
    }
    if (j < E.span) dst[j] = j < E.count ? (float)acc : 0.f;
}

}  // namespace tts

namespace tts_api {

// The tables of a call, fetched so that none is freed while the call still needs it: resample_table empties the handle's cache
// when it is full, so the cache is emptied HERE, once and behind everything that reads the old tables, if the call's missing
// ratios do not fit beside what it holds; then every fetch finds room.
static int rseg_tables(tts_handle_t h, const std::vector<double>& below, bool above, RsegTables* t) {
    auto& rs = h->rs;
    std::vector<double> need;
    if (above) need.push_back(2.0);   // (any ratio above 1 names the shared table)
    need.insert(need.end(), below.begin(), below.end());
    size_t missing = 0;
    for (double rho : need) {
        const ResampleConsts c = resample_consts(rho);
        uint64_t key = 0;
        std::memcpy(&key, &c.scale, sizeof(key));
        missing += rs.tabs.find(key) == rs.tabs.end();
    }
    if (missing && rs.tabs.size() + missing > 32) {
        const int rc = sync_all(h);
        if (rc) return rc;
        resample_release(h);
    }
    for (int k = 0; k < RSEG_TABLES; ++k) t->t[k] = nullptr;
    for (size_t k = 0; k < need.size(); ++k) {
        const double* tab = nullptr;
        const int rc = resample_table(h, need[k], &tab);
        if (rc) return rc;
        t->t[above ? k : k + 1] = reinterpret_cast<const double2*>(tab);
    }
    return TTS_OK;
}

// On h->stream; everything has been checked.  e, tiles, lds: resample_segments_entries' S entries and every launch's tiles and LDS.
static int resample_segments_impl(tts_handle_t h, const float* wav, int n, const std::vector<RsegEntry>& e, const std::vector<int64_t>& tiles,
                                  const std::vector<int>& lds, const RsegTables& tabs, int N_out, float* out) {
    int launches = 0;
    for (int64_t t : tiles) launches += t > 0;
    ProfScope ps(h, ST_RESAMPLE, launches);
    return for_each_segment_launch(e, RSEG_NO_ENTRY, [&](const RsegChunk& c, int ns, int l) -> int {
        if (tiles[(size_t)l] == 0) return TTS_OK;   // (segments that own nothing)
        const int floats = lds[(size_t)l];
        hipLaunchKernelGGL(resample_segments_kernel, dim3((unsigned)tiles[(size_t)l]), dim3(RSEG_TILE), (size_t)floats * sizeof(float), h->stream, wav,
                           out, c, tabs, ns, n, N_out, floats);
        HIPCHK(h, hipGetLastError());
        return TTS_OK;
    });
}

}  // namespace tts_api

extern "C" {

int tts_resample_segments_plan(const tts_resample_segment_t* segments, int S, int B, int n, const int32_t* n_samples, int64_t* n_out) {
    const std::string why = resample_segments_plan(segments, S, B, n, n_samples, n_out);
    return why.empty() ? TTS_OK : fail(nullptr, TTS_ERR_INVALID, "resample_segments_plan: " + why);   // (no handle: tts_last_error(NULL) has the text)
}

int tts_resample_segments(tts_handle_t h, const float* wav, int B, int n, const int32_t* n_samples, const tts_resample_segment_t* segments, int S,
                          int N_out, float* out, int32_t* n_out) {
    DeviceScope dev_scope(h);
    std::string why;
    std::vector<int64_t> rows, count;
    if (!wav || !out || !segments) {
        why = "a NULL pointer (wav, segments and out are required)";
    } else if (N_out < 1) {
        why = "need B, n, S, N_out >= 1";
    } else {
        rows.resize(B > 0 && B <= RSEG_MAX_SEGMENTS ? (size_t)B : 1);   // (the plan refuses B > S before it reads or writes a length)
        count.resize(S > 0 && S <= RSEG_MAX_SEGMENTS ? (size_t)S : 1);
        why = resample_segments_plan(segments, S, B, n, n_samples, rows.data(), count.data());
        if (why == "need B, n, S >= 1") why = "need B, n, S, N_out >= 1";
    }
    if (why.empty()) why = resample_segments_room(rows.data(), B, N_out);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out)) & 3)) why = "the buffers must be 4-byte aligned";
    if (!why.empty()) return fail(h, TTS_ERR_INVALID, "resample_segments: " + why);
    if (!h) return TTS_ERR_INVALID;
    std::vector<double> below;
    bool above = false;
    resample_segments_ratios(segments, S, below, &above);
    RsegTables tabs;
    const int rc = rseg_tables(h, below, above, &tabs);
    if (rc) return rc;
    std::vector<RsegEntry> e;
    std::vector<int64_t> tiles;
    std::vector<int> lds;
    resample_segments_entries(segments, S, n, n_samples, N_out, count.data(), below, e, tiles, lds);
    if (n_out)
        for (int b = 0; b < B; ++b) n_out[b] = (int32_t)rows[(size_t)b];
    return resample_segments_impl(h, wav, n, e, tiles, lds, tabs, N_out, out);
}

int tts_resample_segments_max(void) { return RSEG_MAX_SEGMENTS; }
int tts_resample_segments_max_ratios(void) { return RSEG_MAX_RATIOS; }
int tts_resample_segments_tile(void) { return RSEG_TILE; }

}  // extern "C"
