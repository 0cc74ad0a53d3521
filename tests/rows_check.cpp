// Stand-alone check of the row rules every ragged stage shares (csrc/lengths.h as plain C++, no GPU, no library): the refusal of a
// length outside lo .. hi at both lower bounds, the in/out pair (arithmetic on addresses: no memory is touched) and what fill_lengths
// writes and returns, printed for tests/test_rows_program.py.  Built with -fsanitize=address,undefined where the compiler can.
#include "lengths.h"
#include "check_expect.h"
#include <cstdio>
#include <string>

using namespace tts;

static void pair(const char* name, uintptr_t wav, uintptr_t out, int B, int N) { std::printf("msg %s %s\n", name, in_out_refusal(wav, out, B, N).c_str()); }

template <int CHUNK>
static void filled(const char* name, const int32_t* src, int b0, int nb, int dflt) {
    int dst[CHUNK];
    for (int& d : dst) d = -7;
    const int longest = fill_lengths(dst, src, b0, nb, dflt);
    std::printf("fill %s %d", name, longest);
    for (int d : dst) std::printf(" %d", d);
    std::printf("\n");
}

int main() {
    // the value at index 1 of three, at both lower bounds
    for (int lo : {0, 1})
        for (int v : {-1, 0, 1, 5000, 5001}) {
            const int32_t n[3] = {5000, v, 1};
            const std::string why = lengths_refusal("n_samples", n, 3, "N", 5000, lo);
            std::printf("msg lo%d_%d %s\n", lo, v, why.c_str());
            expect(why == length_refusal("n_samples", 1, v, "N", 5000, lo), "the list's refusal is the one length's");
        }
    expect(lengths_refusal("n_samples", nullptr, 3, "N", 5000, 0).empty() && lengths_refusal("n_samples", nullptr, 3, "N", 5000).empty(), "null: all N");
    const int32_t frames[2] = {0, 3};   // (the bound defaults to 1)
    std::printf("msg default_lo %s\n", lengths_refusal("n_frames", frames, 2, "T", 3).c_str());

    // B = 3 rows of N = 5 floats at 4096: the bytes [4096, 4156)
    const uintptr_t wav = 4096, bytes = 3 * 5 * sizeof(float);
    pair("legal_equal", wav, wav, 3, 5);
    pair("inside_front", wav, wav + sizeof(float), 3, 5);            // out starts one float inside wav
    pair("inside_back", wav, wav + bytes - sizeof(float), 3, 5);     // out starts at wav's last float
    pair("inside_ahead", wav, wav - bytes + sizeof(float), 3, 5);    // out's last float is wav's first
    pair("inside_behind", wav, wav - sizeof(float), 3, 5);           // out starts one float ahead of wav
    pair("legal_adjacent_behind", wav, wav + bytes, 3, 5);
    pair("legal_adjacent_ahead", wav, wav - bytes, 3, 5);
    pair("misaligned_wav", wav + 2, wav + 4 * bytes, 3, 5);
    pair("misaligned_out", wav, wav + 4 * bytes + 2, 3, 5);
    pair("misaligned_and_overlapping", wav, wav + 2, 3, 5);          // (the alignment is reported first)

    const int32_t src[6] = {4, 9, 2, 7, 3, 8};
    filled<4>("full", src, 1, 4, 100);        // src[1 .. 5)
    filled<4>("short_last", src, 4, 2, 100);  // src[4 .. 6), zeros behind
    filled<4>("null", nullptr, 4, 2, 100);    // every row has all of it
    return exit_status();
}
