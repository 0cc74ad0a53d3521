// Dynamic time warping, host side: the cut of an anti-diagonal across the workgroup, the cells of a diagonal, the size of the
// direction-bit workspace and the argument checks of tts_dtw.  Plain C++ (no HIP, no handle): dtw.hip includes it, and
// tests/dtw_check.cpp compiles it alone.
//
// The table of one pair has na x nb cells; diagonal k, 0 <= k <= na + nb - 2, holds the cells (i, k - i) with
// dtw_diag_first(k, nb) <= i <= dtw_diag_last(k, na).  Row i belongs to lane i % DTW_TILE of the pair's workgroup, in its slot
// i / DTW_TILE: a lane keeps its rows for the whole call, so what it needs of the diagonals k - 1 and k - 2 is its own last
// result (left), its upper neighbour's last result (up) and the `up` it read one diagonal earlier (diagonal).
#pragma once
#include "lengths.h"
#include <cstddef>
#include <cstdint>
#include <string>

namespace tts {

constexpr int DTW_TILE = 512;                            // lanes of a workgroup = rows of one slot: the cut along a diagonal
constexpr int DTW_SLOTS = 4;                             // rows a lane owns at most
constexpr int DTW_MAX_FRAMES = DTW_TILE * DTW_SLOTS;     // 2048: two diagonals of (double, int32) are 48 KiB of LDS
constexpr int DTW_MAX_D = 128;
constexpr int DTW_PAIRS = 64;                            // pairs per launch: their lengths travel by value
constexpr int DTW_DIR_CELLS = 16;                        // cells of a table row in one 32-bit word of direction bits, 2 bits each
// the direction codes: where the best predecessor of a cell lies
constexpr unsigned DTW_DIAG = 0, DTW_UP = 1, DTW_LEFT = 2, DTW_START = 3;

// (constexpr: the kernel calls these too)
constexpr int dtw_diagonals(int na, int nb) { return na + nb - 1; }
// first and last row i of diagonal k (the diagonal is empty where first > last: k < 0 or k > na + nb - 2)
constexpr int dtw_diag_first(int k, int nb) { return k - (nb - 1) > 0 ? k - (nb - 1) : 0; }
constexpr int dtw_diag_last(int k, int na) { return k < na - 1 ? k : na - 1; }
// the slots of a lane that can hold a row at all: ceil(na / DTW_TILE)
constexpr int dtw_slots(int na) { return (na + DTW_TILE - 1) / DTW_TILE; }

// direction bits: row i of a pair is dtw_dir_words(cols) words, a pair dtw_dir_pair_words(rows, cols); rows / cols: the longest
// na / nb of the call
inline size_t dtw_dir_words(int cols) { return (size_t)((cols + DTW_DIR_CELLS - 1) / DTW_DIR_CELLS); }
inline size_t dtw_dir_pair_words(int rows, int cols) { return (size_t)rows * dtw_dir_words(cols); }
inline size_t dtw_dir_bytes(int B, int rows, int cols) { return (size_t)B * dtw_dir_pair_words(rows, cols) * sizeof(uint32_t); }

// The checks of tts_dtw, in the order the header lists them.  An empty string: the call is legal.  *unsupported is set where the
// refusal is a length above DTW_MAX_FRAMES or a D above DTW_MAX_D (TTS_ERR_UNSUPPORTED), cleared otherwise (TTS_ERR_INVALID).
// n_a / n_b: host lengths or null (all Ta / Tb).  *rows / *cols: the longest na / nb.
inline std::string dtw_check(bool have_ptrs, int Ta, int stride_a, const int32_t* n_a, int Tb, int stride_b, const int32_t* n_b, int B, int D,
                             bool* unsupported, int* rows, int* cols) {
    *unsupported = false;
    *rows = *cols = 0;
    if (!have_ptrs) return "a NULL pointer (a, b, cost and path_len are required)";
    if (B < 1 || Ta < 1 || Tb < 1 || D < 1) return "need B, Ta, Tb, D >= 1";
    if (stride_a < D || stride_b < D) return "a row stride smaller than D";
    int longest_a = 0, longest_b = 0;
    for (int p = 0; p < B; ++p) {
        const int na = n_a ? n_a[p] : Ta, nb = n_b ? n_b[p] : Tb;
        std::string why = length_refusal("n_a", p, na, "Ta", Ta);   // (pair by pair, a ahead of b)
        if (why.empty()) why = length_refusal("n_b", p, nb, "Tb", Tb);
        if (!why.empty()) return why;
        longest_a = na > longest_a ? na : longest_a;
        longest_b = nb > longest_b ? nb : longest_b;
    }
    *rows = longest_a;
    *cols = longest_b;
    if (D > DTW_MAX_D) {
        *unsupported = true;
        return "D = " + std::to_string(D) + " is larger than " + std::to_string(DTW_MAX_D);
    }
    if (longest_a > DTW_MAX_FRAMES || longest_b > DTW_MAX_FRAMES) {
        *unsupported = true;
        return "a sequence of " + std::to_string(longest_a > longest_b ? longest_a : longest_b) + " frames is longer than tts_dtw_max_frames() = " +
               std::to_string(DTW_MAX_FRAMES);
    }
    return std::string();
}

}  // namespace tts
