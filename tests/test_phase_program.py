"""The host side of the estimated initial phases (csrc/phase_plan.h: the cut of the frames into chunks and the argument checks of the estimate's entry
points) as a stand-alone host program: tests/phase_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer
and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  Its
chunk counts are held against the same arithmetic here.  No GPU, nothing loaded into Python."""
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_phase_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('phase_check.cpp', tmp_path)[0])
    chunk = int(rows[0][0])
    assert chunk >= 1 and len(rows) == 1 + 4 * chunk + 3
    for n, count in rows[1:]:
        assert int(count) == (0 if int(n) < 1 else -(-int(n) // chunk)), (n, count)
    assert refusals == {'n_frames=%d' % n: LENGTH_REFUSAL.format(name='n_frames', b=1, n=n, bound='T', hi=12) for n in (0, -1, 13)}
