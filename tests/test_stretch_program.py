"""The host side of the speaking-rate feature (csrc/stretch_plan.h: the frame count and the argument checks of the stretch entry
points) as a stand-alone host program: tests/stretch_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer
and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  Its
frame counts are held against numpy here.  No GPU, nothing loaded into Python."""
import numpy as np

from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_stretch_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('stretch_check.cpp', tmp_path)[0])
    assert len(rows) == 10 * 64
    for n, r, count in rows:
        assert int(count) == len(np.arange(0, int(n), float(r), dtype=float)), (n, r, count)
    assert refusals == {'n_frames=%d' % n: LENGTH_REFUSAL.format(name='n_frames', b=1, n=n, bound='T', hi=12) for n in (0, -1, 13)}
