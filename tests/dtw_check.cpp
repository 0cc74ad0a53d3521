// Stand-alone check of the host side of mel-cepstral distortion (csrc/dtw_plan.h and csrc/cepstrum_plan.h compiled as plain C++, no
// GPU, no library): prints the cut, the cells of every anti-diagonal, the rows of the lanes' slots and the direction-bit workspace
// of a grid of table shapes, what tts_dtw and tts_mfcc answer to a list of argument sets, and samples of the DCT table, for
// tests/test_dtw_program.py to hold against the numpy oracles.  Built with -fsanitize=address,undefined where the compiler has
// the runtimes.
#include "cepstrum_plan.h"
#include "dtw_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

static std::string g_why;   // the refusal text of the last dtw_answer

// 0: legal, 1: TTS_ERR_INVALID, 2: TTS_ERR_UNSUPPORTED
static int dtw_answer(bool ptrs, int Ta, int sa, const std::vector<int32_t>* na, int Tb, int sb, const std::vector<int32_t>* nb, int B, int D,
                      int* rows = nullptr, int* cols = nullptr) {
    bool unsupported = false;
    int r = 0, c = 0;
    const std::string why = dtw_check(ptrs, Ta, sa, na ? na->data() : nullptr, Tb, sb, nb ? nb->data() : nullptr, B, D, &unsupported, &r, &c);
    g_why = why;
    if (rows) *rows = r;
    if (cols) *cols = c;
    expect(why.empty() ? !unsupported : true, "unsupported is set with a reason only");
    return why.empty() ? 0 : unsupported ? 2 : 1;
}

static bool mfcc_refused(bool ptrs, int B, int T, int n_mels, int stride, const std::vector<int32_t>* n, int n_mfcc) {
    return !mfcc_check(ptrs, B, T, n_mels, stride, n ? n->data() : nullptr, n_mfcc).empty();
}

int main() {
    const int t = DTW_TILE;
    std::printf("consts %d %d %d %d %d %d\n", DTW_TILE, DTW_SLOTS, DTW_MAX_FRAMES, DTW_MAX_D, DTW_PAIRS, DTW_DIR_CELLS);
    expect(DTW_MAX_FRAMES >= 2048 && DTW_MAX_FRAMES == DTW_TILE * DTW_SLOTS, "the longest sequence");
    expect(2 * (size_t)DTW_MAX_FRAMES * (sizeof(double) + sizeof(int32_t)) <= 48 * 1024, "two diagonals fit 48 KiB of LDS");

    const std::vector<int> sizes = {1, 2, 9, t - 1, t, t + 1};
    for (int na : sizes)
        for (int nb : sizes) {
            const int nd = dtw_diagonals(na, nb);
            std::printf("shape %d %d %d %d\n", na, nb, nd, dtw_slots(na));
            long long cells = 0;
            for (int k = -1; k <= nd; ++k) {
                const int lo = dtw_diag_first(k, nb), hi = dtw_diag_last(k, na);
                std::printf("diag %d %d %d %d %d\n", na, nb, k, lo, hi);
                if (k >= 0 && k < nd) {
                    expect(lo <= hi && lo >= 0 && hi < na && k - lo < nb && k - hi >= 0, "a diagonal inside the table");
                    expect(hi / DTW_TILE < dtw_slots(na), "every row of a diagonal has a slot");
                    cells += hi - lo + 1;
                } else {
                    expect(lo > hi, "no cells outside the table");
                }
            }
            expect(cells == (long long)na * nb, "the diagonals cover the table once");
        }
    for (int na : {1, t - 1, t, t + 1, 2 * t, 2 * t + 3, DTW_MAX_FRAMES}) std::printf("slots %d %d\n", na, dtw_slots(na));
    expect(dtw_slots(DTW_MAX_FRAMES) == DTW_SLOTS, "the longest sequence fills the slots");

    for (int B : {1, 5, 64})
        for (int rows : {1, 9, t + 1, DTW_MAX_FRAMES})
            for (int cols : {1, 15, 16, 17, t + 1, DTW_MAX_FRAMES})
                std::printf("dir %d %d %d %zu %zu %zu\n", B, rows, cols, dtw_dir_words(cols), dtw_dir_pair_words(rows, cols), dtw_dir_bytes(B, rows, cols));

    // ---- tts_dtw's answers
    const std::vector<int32_t> la = {12, 7, 1}, lb = {3, 20, 20};
    int rows = 0, cols = 0;
    std::printf("dtw_check legal_ragged %d\n", dtw_answer(true, 12, 14, &la, 20, 13, &lb, 3, 13, &rows, &cols));
    expect(rows == 12 && cols == 20, "the longest lengths of a ragged call");
    std::printf("dtw_check legal_uniform %d\n", dtw_answer(true, 12, 13, nullptr, 20, 13, nullptr, 3, 13, &rows, &cols));
    expect(rows == 12 && cols == 20, "the longest lengths of a uniform call");
    std::printf("dtw_check legal_1x1 %d\n", dtw_answer(true, 1, 1, nullptr, 1, 1, nullptr, 1, 1));
    std::printf("dtw_check legal_longest %d\n", dtw_answer(true, DTW_MAX_FRAMES, DTW_MAX_D, nullptr, DTW_MAX_FRAMES, DTW_MAX_D, nullptr, 2, DTW_MAX_D));
    {   // padded buffers beyond the limit are legal while the lengths are not
        const std::vector<int32_t> a1 = {DTW_MAX_FRAMES}, b1 = {5};
        std::printf("dtw_check legal_long_padding %d\n", dtw_answer(true, DTW_MAX_FRAMES + 100, 2, &a1, 9, 2, &b1, 1, 2));
    }
    std::printf("dtw_check null %d\n", dtw_answer(false, 12, 13, nullptr, 20, 13, nullptr, 3, 13));
    std::printf("dtw_check B0 %d\n", dtw_answer(true, 12, 13, nullptr, 20, 13, nullptr, 0, 13));
    std::printf("dtw_check Ta0 %d\n", dtw_answer(true, 0, 13, nullptr, 20, 13, nullptr, 3, 13));
    std::printf("dtw_check Tb0 %d\n", dtw_answer(true, 12, 13, nullptr, -1, 13, nullptr, 3, 13));
    std::printf("dtw_check D0 %d\n", dtw_answer(true, 12, 13, nullptr, 20, 13, nullptr, 3, 0));
    std::printf("dtw_check stride_a %d\n", dtw_answer(true, 12, 12, nullptr, 20, 13, nullptr, 3, 13));
    std::printf("dtw_check stride_b %d\n", dtw_answer(true, 12, 13, nullptr, 20, 12, nullptr, 3, 13));
    for (int bad : {0, -1, 13}) {
        std::vector<int32_t> l = la;
        l[2] = bad;
        std::printf("dtw_check n_a=%d %d\n", bad, dtw_answer(true, 12, 13, &l, 20, 13, &lb, 3, 13));
        std::printf("msg n_a=%d %s\n", bad, g_why.c_str());
    }
    for (int bad : {0, -5, 21}) {
        std::vector<int32_t> l = lb;
        l[0] = bad;
        std::printf("dtw_check n_b=%d %d\n", bad, dtw_answer(true, 12, 13, &la, 20, 13, &l, 3, 13));
        std::printf("msg n_b=%d %s\n", bad, g_why.c_str());
    }
    {   // the lengths are checked pair by pair, n_a[p] ahead of n_b[p]: the first refusal is the earlier pair's
        const std::vector<int32_t> a2 = {12, 7, 0}, b2 = {0, 20, 20}, a3 = {12, 0, 1}, b3 = {3, 21, 20};
        dtw_answer(true, 12, 13, &a2, 20, 13, &b2, 3, 13);
        std::printf("msg order_pairs %s\n", g_why.c_str());
        dtw_answer(true, 12, 13, &a3, 20, 13, &b3, 3, 13);
        std::printf("msg order_sides %s\n", g_why.c_str());
    }
    std::printf("dtw_check D_above %d\n", dtw_answer(true, 12, 200, nullptr, 20, 200, nullptr, 3, DTW_MAX_D + 1));
    std::printf("dtw_check Ta_above %d\n", dtw_answer(true, DTW_MAX_FRAMES + 1, 13, nullptr, 20, 13, nullptr, 1, 13));
    std::printf("dtw_check Tb_above %d\n", dtw_answer(true, 20, 13, nullptr, DTW_MAX_FRAMES + 1, 13, nullptr, 1, 13));
    {
        const std::vector<int32_t> a1 = {3, DTW_MAX_FRAMES + 1}, b1 = {5, 5};
        std::printf("dtw_check n_a_above %d\n", dtw_answer(true, DTW_MAX_FRAMES + 100, 2, &a1, 9, 2, &b1, 2, 2));
    }

    // ---- tts_mfcc's answers
    const std::vector<int32_t> lf = {12, 7, 1};
    expect(!mfcc_refused(true, 3, 12, 80, 80, &lf, 13), "a legal ragged call");
    expect(!mfcc_refused(true, 3, 12, 80, 96, nullptr, 80), "a legal call on padded rows, every coefficient");
    expect(!mfcc_refused(true, 1, 1, 1, 1, nullptr, 1), "the smallest call");
    expect(!mfcc_refused(true, 1, 1, MFCC_MAX_MELS, MFCC_MAX_MELS, nullptr, MFCC_MAX_MELS), "the widest call");
    expect(mfcc_refused(false, 3, 12, 80, 80, nullptr, 13), "NULL pointer");
    expect(mfcc_refused(true, 0, 12, 80, 80, nullptr, 13) && mfcc_refused(true, 3, 0, 80, 80, nullptr, 13), "B, T below 1");
    expect(mfcc_refused(true, 3, 12, 0, 80, nullptr, 13) && mfcc_refused(true, 3, 12, 80, 80, nullptr, 0), "n_mels, n_mfcc below 1");
    expect(mfcc_refused(true, 3, 12, MFCC_MAX_MELS + 1, MFCC_MAX_MELS + 1, nullptr, 13), "n_mels above the limit");
    expect(mfcc_refused(true, 3, 12, 80, 80, nullptr, 81), "n_mfcc > n_mels");
    expect(mfcc_refused(true, 3, 12, 80, 79, nullptr, 13), "row_stride < n_mels");
    for (int bad : {0, -1, 13}) {
        std::vector<int32_t> l = lf;
        l[1] = bad;
        expect(mfcc_refused(true, 3, 12, 80, 80, &l, 13), "n_frames outside [1, T]");
        std::printf("msg n_frames=%d %s\n", bad, mfcc_check(true, 3, 12, 80, 80, l.data(), 13).c_str());
    }

    // ---- the DCT table, laid out [n][k]
    for (int n_mels : {1, 16, 80, 1024})
        for (int n_mfcc : {1, 13, n_mels}) {
            if (n_mfcc > n_mels) continue;
            const std::vector<double> tab = mfcc_table(n_mels, n_mfcc);
            expect(tab.size() == (size_t)n_mels * n_mfcc, "the table's size");
            for (int n : {0, 1, n_mels / 2, n_mels - 1})
                for (int k : {0, 1, n_mfcc / 2, n_mfcc - 1})
                    if (n >= 0 && n < n_mels && k >= 0 && k < n_mfcc) std::printf("tab %d %d %d %d %.17g\n", n_mels, n_mfcc, n, k, tab[(size_t)n * n_mfcc + k]);
        }
    return exit_status();
}
