// Batched dynamic time warping of two feature sequences: the alignment under mel-cepstral distortion (audio/metrics.py).
// No reference counterpart.  For one pair with na and nb frames of D floats (include/sstts_hip.h has the definition in full):
//   c(i, j)  = sqrt(sum_d ((double)a[i][d] - (double)b[j][d])^2), d ascending, every operation an IEEE double operation of its own
//   Dm(i, j) = c(i, j) + Dm(best), L(i, j) = L(best) + 1; best: the first of diagonal, up, left that exists, replaced by a later
//              one iff that one's Dm is strictly smaller
// and cost = Dm(na - 1, nb - 1), path_len = L(na - 1, nb - 1), path = the chain of `best` from (0, 0).
// One workgroup per pair walks the na + nb - 1 anti-diagonals, a barrier behind each.  Row i of the table belongs to lane
// i % DTW_TILE for the whole call (dtw_plan.h), so of the three predecessors of a cell a lane holds two in registers -- its own
// last result (left) and the `up` it read one diagonal ago (diagonal) -- and reads one, the upper neighbour's last result, from
// LDS: two diagonals of (double, int32), 48 KiB.  Local costs are computed on the fly; with D <= 16 a lane keeps its rows of `a`
// in registers.  With a path the lane packs the direction of 16 cells of its row into a word of the workspace "dtw.dir"; lane 0
// then walks back at most na + nb - 1 steps.  No atomics; every loop bound is a host length that travelled in the launch.
#include "api_internal.h"
#include "dtw_plan.h"

// s = s + t * t is a product and a sum (tests/dtw_oracle.py); the file is also built with -ffp-contract=off (build.py)
#pragma clang fp contract(off)

namespace tts {

constexpr int DTW_CACHE_D = 16;   // D up to which a lane keeps its rows of `a` in registers

struct DtwLens {
    int na[DTW_PAIRS];
    int nb[DTW_PAIRS];
};

// a, b, cost, path_len, path and dir point at the first pair of the launch.  pair_a / pair_b: floats between two pairs; path_rows
// = Ta + Tb - 1; dir: null without a path, else dir_pair words per pair in rows of dir_row words.
template <bool CACHE_A>
__global__ __launch_bounds__(DTW_TILE) void dtw_kernel(const float* __restrict__ a, size_t pair_a, int stride_a, const float* __restrict__ b,
                                                       size_t pair_b, int stride_b, DtwLens lens, int D, double* __restrict__ cost,
                                                       int32_t* __restrict__ path_len, int32_t* __restrict__ path, size_t path_rows,
                                                       uint32_t* __restrict__ dir, size_t dir_pair, int dir_row) {
    __shared__ double sD[2][DTW_MAX_FRAMES];
    __shared__ int sL[2][DTW_MAX_FRAMES];
    __shared__ int s_len;
    const int p = blockIdx.x, t = threadIdx.x;
    const int na = lens.na[p], nb = lens.nb[p];
    const float* A = a + (size_t)p * pair_a;
    const float* Bm = b + (size_t)p * pair_b;
    uint32_t* dirp = dir ? dir + (size_t)p * dir_pair : nullptr;
    const int slots = dtw_slots(na);   // (uniform)
    double leftD[DTW_SLOTS], diagD[DTW_SLOTS];
    int leftL[DTW_SLOTS], diagL[DTW_SLOTS];
    uint32_t acc[DTW_SLOTS];
    float ar[DTW_SLOTS][CACHE_A ? DTW_CACHE_D : 1];
#pragma unroll
    for (int s = 0; s < DTW_SLOTS; ++s) {
        leftD[s] = diagD[s] = 0.0;
        leftL[s] = diagL[s] = 0;
        acc[s] = 0u;
        const int i = t + s * DTW_TILE;
        if (CACHE_A) {
#pragma unroll
            for (int d = 0; d < DTW_CACHE_D; ++d) ar[s][d] = (i < na && d < D) ? A[(size_t)i * stride_a + d] : 0.f;
        }
    }
    const int n_diag = dtw_diagonals(na, nb);
    for (int k = 0; k < n_diag; ++k) {
        const int cur = k & 1, prev = cur ^ 1;
#pragma unroll
        for (int s = 0; s < DTW_SLOTS; ++s) {
            const int i = t + s * DTW_TILE, j = k - i;
            if (s < slots && i < na && j >= 0 && j < nb) {
                const float* br = Bm + (size_t)j * stride_b;
                double sum = 0.0;
                if (CACHE_A) {
#pragma unroll
                    for (int d = 0; d < DTW_CACHE_D; ++d)
                        if (d < D) {
                            const double df = __dsub_rn((double)ar[s][d], (double)br[d]);
                            sum = __dadd_rn(sum, __dmul_rn(df, df));
                        }
                } else {
                    const float* arow = A + (size_t)i * stride_a;
                    for (int d = 0; d < D; ++d) {
                        const double df = __dsub_rn((double)arow[d], (double)br[d]);
                        sum = __dadd_rn(sum, __dmul_rn(df, df));
                    }
                }
                const double c = __dsqrt_rn(sum);
                double upD = 0.0;
                int upL = 0;
                if (i > 0) {
                    upD = sD[prev][i - 1];
                    upL = sL[prev][i - 1];
                }
                double best = 0.0;
                int bl = 0;
                unsigned code = DTW_START;
                if (i > 0 && j > 0) {
                    best = diagD[s], bl = diagL[s], code = DTW_DIAG;
                    if (upD < best) best = upD, bl = upL, code = DTW_UP;
                    if (leftD[s] < best) best = leftD[s], bl = leftL[s], code = DTW_LEFT;
                } else if (i > 0) {
                    best = upD, bl = upL, code = DTW_UP;
                } else if (j > 0) {
                    best = leftD[s], bl = leftL[s], code = DTW_LEFT;
                }
                const double dm = code == DTW_START ? c : __dadd_rn(c, best);
                const int len = bl + 1;
                sD[cur][i] = dm;
                sL[cur][i] = len;
                leftD[s] = dm;
                leftL[s] = len;
                diagD[s] = upD;
                diagL[s] = upL;
                if (dirp) {
                    acc[s] |= code << (2 * (j & (DTW_DIR_CELLS - 1)));
                    if ((j & (DTW_DIR_CELLS - 1)) == DTW_DIR_CELLS - 1 || j == nb - 1) {
                        dirp[(size_t)i * dir_row + j / DTW_DIR_CELLS] = acc[s];
                        acc[s] = 0u;
                    }
                }
                if (i == na - 1 && j == nb - 1) {
                    cost[p] = dm;
                    path_len[p] = len;
                    s_len = len;
                }
            }
        }
        __syncthreads();
    }
    if (!path) return;
    // the path: rows behind it are (-1, -1); lane 0 walks the directions back from the last cell, at most n_diag steps
    int32_t* P = path + (size_t)p * path_rows * 2;
    const int L = min(max(s_len, 1), n_diag);
    for (size_t r = (size_t)L + t; r < path_rows; r += DTW_TILE) {
        P[2 * r] = -1;
        P[2 * r + 1] = -1;
    }
    if (t == 0) {
        int i = na - 1, j = nb - 1, wi = -1, wj = -1;
        uint32_t w = 0u;
        for (int pos = L - 1; pos >= 0; --pos) {
            P[2 * (size_t)pos] = i;
            P[2 * (size_t)pos + 1] = j;
            if (i != wi || j / DTW_DIR_CELLS != wj) {
                wi = i, wj = j / DTW_DIR_CELLS;
                w = dirp[(size_t)wi * dir_row + wj];
            }
            const unsigned code = (w >> (2 * (j & (DTW_DIR_CELLS - 1)))) & 3u;
            if (code == DTW_DIAG && i > 0 && j > 0) --i, --j;
            else if (code == DTW_UP && i > 0) --i;
            else if (code == DTW_LEFT && j > 0) --j;
            else break;   // (0, 0)
        }
    }
}

}  // namespace tts

namespace tts_api {

// On h->stream.  n_a / n_b: HOST lengths or null (all Ta / Tb); everything has been checked (dtw_check), rows / cols are the
// longest na / nb it found.
static int dtw_impl(tts_handle_t h, const float* a, int Ta, int stride_a, const int32_t* n_a, const float* b, int Tb, int stride_b,
                    const int32_t* n_b, int B, int D, double* cost, int32_t* path_len, int32_t* path, int rows, int cols) {
    uint32_t* dir = nullptr;
    const size_t dir_pair = dtw_dir_pair_words(rows, cols);
    if (path) {
        WS(h, "dtw.dir", uint32_t, (size_t)B * dir_pair, d);
        dir = d;
    }
    ProfScope ps(h, ST_DTW, length_chunks(B, DTW_PAIRS));
    const size_t pair_a = (size_t)Ta * stride_a, pair_b = (size_t)Tb * stride_b, path_rows = (size_t)Ta + Tb - 1;
    for (int p0 = 0; p0 < B; p0 += DTW_PAIRS) {
        const int np = std::min(DTW_PAIRS, B - p0);
        DtwLens lens;
        fill_lengths(lens.na, n_a, p0, np, Ta);
        fill_lengths(lens.nb, n_b, p0, np, Tb);
        const float* pa = a + (size_t)p0 * pair_a;
        const float* pb = b + (size_t)p0 * pair_b;
        int32_t* pp = path ? path + (size_t)p0 * path_rows * 2 : nullptr;
        uint32_t* pd = dir ? dir + (size_t)p0 * dir_pair : nullptr;
        if (D <= DTW_CACHE_D)
            hipLaunchKernelGGL(dtw_kernel<true>, dim3(np), dim3(DTW_TILE), 0, h->stream, pa, pair_a, stride_a, pb, pair_b, stride_b, lens, D,
                               cost + p0, path_len + p0, pp, path_rows, pd, dir_pair, (int)dtw_dir_words(cols));
        else
            hipLaunchKernelGGL(dtw_kernel<false>, dim3(np), dim3(DTW_TILE), 0, h->stream, pa, pair_a, stride_a, pb, pair_b, stride_b, lens, D,
                               cost + p0, path_len + p0, pp, path_rows, pd, dir_pair, (int)dtw_dir_words(cols));
        HIPCHK(h, hipGetLastError());
    }
    return TTS_OK;
}

}  // namespace tts_api

extern "C" {

int tts_dtw(tts_handle_t h, const float* a, int Ta, int stride_a, const int32_t* n_a, const float* b, int Tb, int stride_b, const int32_t* n_b,
            int B, int D, double* cost, int32_t* path_len, int32_t* path) {
    DeviceScope dev_scope(h);
    bool unsupported = false;
    int rows = 0, cols = 0;
    std::string why = dtw_check(a && b && cost && path_len, Ta, stride_a, n_a, Tb, stride_b, n_b, B, D, &unsupported, &rows, &cols);
    if (why.empty() && ((reinterpret_cast<uintptr_t>(cost) & 7) || ((reinterpret_cast<uintptr_t>(path_len) | reinterpret_cast<uintptr_t>(path)) & 3) ||
                        ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3)))
        why = "cost must be 8-byte aligned, the other buffers 4-byte aligned";
    if (!why.empty()) return fail(h, unsupported ? TTS_ERR_UNSUPPORTED : TTS_ERR_INVALID, "dtw: " + why);
    if (!h) return TTS_ERR_INVALID;
    return dtw_impl(h, a, Ta, stride_a, n_a, b, Tb, stride_b, n_b, B, D, cost, path_len, path, rows, cols);
}

int tts_dtw_max_frames(void) { return DTW_MAX_FRAMES; }

int tts_dtw_tile(void) { return DTW_TILE; }

}  // extern "C"
