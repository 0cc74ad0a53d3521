"""The host side of the persistent decoders' hand-off (csrc/decoder_cluster.h: the layout of a launch's sync words and the
window arithmetic of LocalLuongAttention) as a stand-alone host program: tests/decoder_cluster_check.cpp with its own main,
compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the
program needs nothing preloaded) -- and run.  The program writes every word its view hands out in a buffer of exactly the
word count; what it prints is held against the layout as DESIGN.md states it.  No GPU, nothing loaded into Python."""
from host_checks import build_and_run


def test_decoder_cluster_check_program(tmp_path):
    rows = build_and_run('decoder_cluster_check.cpp', tmp_path)[0]
    layouts = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == 'layout']
    assert len(layouts) == 8 * 11
    assert {(c, s) for c, s, *_ in layouts} == {(c, s) for c in range(1, 9) for s in range(11)}   # below, at and above the launch's
    for clusters, sync_clusters, laid_out, words, resident, status in layouts:
        # 64 words per cluster of the larger count, then the resident count, then the status word
        assert laid_out == max(clusters, sync_clusters)
        assert (resident, status, words) == (64 * laid_out, 64 * laid_out + 1, 64 * laid_out + 2)
