// Stand-alone check of the host side of the persistent decoders' hand-off (csrc/decoder_cluster.h compiled as plain C++, no GPU,
// no library): the layout of a launch's sync words -- for 1 to 8 clusters, laid out for a cluster count below, at and above the
// launch's own -- and the monotonic window of LocalLuongAttention.  Every word the view hands out is written in a buffer of
// exactly dc_sync_words() words.  Built with -fsanitize=address,undefined where the compiler has the runtimes.
#include "decoder_cluster.h"
#include "check_expect.h"
#include <cstdio>
#include <vector>

using namespace tts;

int main() {
    int layouts = 0;
    for (int clusters = 1; clusters <= 8; ++clusters)
        for (int sync_clusters = 0; sync_clusters <= 10; ++sync_clusters) {
            const int lc = dc_layout_clusters(clusters, sync_clusters);
            expect(lc >= clusters && lc >= sync_clusters && (lc == clusters || lc == sync_clusters), "the layout is that of the larger count");
            const size_t words = dc_sync_words(lc);
            std::vector<unsigned> buf(words, 0u);
            const DcSync v = dc_sync(buf.data(), lc);
            // every index handed out lies inside the buffer, and no two of them are the same word
            expect(v.counters == buf.data(), "the counters come first");
            for (int c = 0; c < lc; ++c) {
                unsigned* cnt = v.counters + (size_t)DC_CNT_LD * c;
                expect(cnt + 1 <= buf.data() + words, "a counter lies inside the buffer");
                if (c > 0) expect(cnt - (v.counters + (size_t)DC_CNT_LD * (c - 1)) == 64, "counters are 64 words apart");
                *cnt += 1u;
            }
            expect(v.resident - buf.data() == (long)dc_resident_index(lc) && dc_resident_index(lc) < words, "the resident count lies inside the buffer");
            expect(reinterpret_cast<unsigned*>(v.status) - buf.data() == (long)dc_status_index(lc) && dc_status_index(lc) < words,
                   "the status word lies inside the buffer");
            expect(v.resident > v.counters + (size_t)DC_CNT_LD * (lc - 1), "the resident count is behind the last counter");
            expect(reinterpret_cast<unsigned*>(v.status) == v.resident + 1, "the status word is behind the resident count");
            *v.resident += 1u;
            *v.status += 1;
            size_t written = 0;
            for (size_t i = 0; i < words; ++i) {
                expect(buf[i] <= 1u, "no word was handed out twice");
                written += buf[i];
            }
            expect(written == (size_t)lc + 2, "clusters + 2 distinct words");
            // what a launch zeroes ends in front of the sticky status word and covers everything else
            expect(dc_zeroed_words(lc) == dc_status_index(lc) && dc_zeroed_words(lc) == dc_resident_index(lc) + 1, "zeroed: all but the status word");
            std::printf("layout %d %d %d %zu %zu %zu\n", clusters, sync_clusters, lc, words, dc_resident_index(lc), dc_status_index(lc));
            ++layouts;
        }
    expect(layouts == 88, "8 x 11 layouts");

    // the monotonic window [c - D, c + D + 1) stays inside a memory of Ts >= 2D + 1 positions and follows the step in between
    for (int D = 1; D <= 5; ++D)
        for (int Ts = 2 * D + 1; Ts <= 2 * D + 9; ++Ts)
            for (int t = 0; t < Ts + 4; ++t) {
                const int c = local_center(t, Ts, D);
                expect(local_inside_memory(c, D, Ts), "the monotonic window is inside the memory");
                expect(local_clamped_lo(c, D, Ts, 2 * D + 1) == c - D, "a window inside the memory is not moved by the clamp");
                if (t >= D && t <= Ts - (D + 1)) expect(c == t, "the centre is the step");
            }
    // a predicted window that leaves the memory is clamped into it
    expect(!local_inside_memory(1, 2, 20) && local_clamped_lo(1, 2, 20, 5) == 0, "left edge");
    expect(!local_inside_memory(18, 2, 20) && local_clamped_lo(18, 2, 20, 5) == 15, "right edge");
    expect(local_inside_memory(17, 2, 20) && local_clamped_lo(17, 2, 20, 5) == 15, "the last window inside");
    return exit_status();
}
