// Stand-alone check of the host side of the estimated initial phases (csrc/phase_plan.h compiled as plain C++, no GPU, no
// library): prints the chunk counts of a range of lengths for tests/test_phase_program.py to hold against its own arithmetic, and
// runs the argument checks of the estimate's entry points through every refusal the header lists.  Built with
// -fsanitize=address,undefined where the compiler has the runtimes.
#include "phase_plan.h"
#include "check_expect.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace tts;

static bool refused(bool ptrs, int B, int T, int stride, const int32_t* n, int n_fft, int hop) {
    return !phase_check(ptrs, B, T, stride, n, n_fft, hop).empty();
}

int main() {
    std::printf("%d\n", PE_CHUNK);
    for (int n = -1; n <= 4 * PE_CHUNK + 1; ++n) std::printf("%d %d\n", n, pe_chunks(n));
    expect(pe_chunks(PE_MAX_FRAMES) == PE_MAX_FRAMES / PE_CHUNK, "the longest utterance's chunks");

    for (int n_fft : {256, 512, 1024, 2048, 4096}) expect(pe_nfft_ok(n_fft), "a legal n_fft");
    for (int n_fft : {0, -256, 128, 255, 257, 1000, 3000, 8192, 1 << 30}) expect(!pe_nfft_ok(n_fft), "an illegal n_fft");

    const int B = 3, T = 12, F = 1025;
    const std::vector<int32_t> lens = {12, 7, 1};
    expect(!refused(true, B, T, F, lens.data(), 2048, 275), "a legal ragged call");
    expect(!refused(true, B, T, F + 31, nullptr, 2048, 275), "a legal uniform call on padded rows");
    expect(!refused(true, 1, 1, 129, nullptr, 256, 256), "one frame, hop = n_fft");
    expect(!refused(true, 1, PE_MAX_FRAMES, 129, nullptr, 256, 1), "the longest legal utterance");
    expect(refused(false, B, T, F, nullptr, 2048, 275), "NULL pointer");
    for (int n_fft : {0, 128, 1000, 8192}) expect(refused(true, B, T, 1 + n_fft / 2, nullptr, n_fft, 64), "bad n_fft");
    for (int hop : {0, -1, 2049}) expect(refused(true, B, T, F, nullptr, 2048, hop), "bad hop_length");
    expect(refused(true, 0, T, F, nullptr, 2048, 275) && refused(true, B, 0, F, nullptr, 2048, 275), "B, T below 1");
    expect(refused(true, 1, PE_MAX_FRAMES + 1, F, nullptr, 2048, 275), "T beyond the limit");
    expect(refused(true, B, T, F - 1, nullptr, 2048, 275), "row_stride < F");
    for (int bad : {0, -1, T + 1}) {
        std::vector<int32_t> l = lens;
        l[1] = bad;
        expect(refused(true, B, T, F, l.data(), 2048, 275), "n_frames outside [1, T]");
        std::printf("msg n_frames=%d %s\n", bad, phase_check(true, B, T, F, l.data(), 2048, 275).c_str());
    }
    return exit_status();
}
