"""tts_limit and tts_true_peak beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the
manner of tests/test_gpu_loudness_neighbours.py -- a server limits one batch while a second engine may be busy on the same chip.
csrc/limiter.hip: double arithmetic, shuffles and integer atomics on bit patterns, no packed float32 arithmetic."""
import numpy as np
import pytest

import limiter_cases as C
import limiter_oracle as O
from conftest import pkg
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_limiter_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    L, B = 110, 16
    lens = np.array([3 * O.TILE + 91 - 301 * b for b in range(B)], np.int32)
    rows = [C.kitchen(int(n), L) if b % 4 else C.quiet(int(n)) for b, n in enumerate(lens)]
    X, _ = C.padded(rows, np.nan)
    d_x = engine.to_device(X)

    def run():
        tp, sp = engine.true_peak(d_x, n_samples=lens, want_sample_peak=True)
        work = engine.to_device(X)
        out, stats = engine.limit(work, C.CEILING, L, 4, n_samples=lens)
        y = out.to_host()
        work.free()
        return tp, sp, stats, y

    try:
        ref = run()
        # ... and the quiet run is right: three utterances against the oracle
        taps = pkg('_hip').true_peak_filter()
        for b in (0, 1, 11):
            want, st = O.limit(rows[b], taps, C.CEILING, L, 4)
            assert np.array_equal(C.bits(ref[3][b, :lens[b]]), C.bits(want)) and tuple(ref[2][b]) == st
            assert (ref[0][b], ref[1][b]) == O.true_peak(rows[b], taps)
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes() and
                        np.array_equal(C.bits(got[3]), C.bits(ref[3])))
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d_x.free()
