"""tts_loudness and tts_loudness_normalize beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as
alone, in the manner of tests/test_gpu_f0_neighbours.py -- a server normalises one batch while a second engine may be busy on the
same chip.  csrc/loudness.hip: double arithmetic, shuffles and an integer maximum, no packed float32 arithmetic."""
import numpy as np
import pytest

import loudness_cases as C
import loudness_oracle as O
from conftest import pkg
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_loudness_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    s = O.step(C.SR)
    B = 16
    lens = np.array([12 * s + 91 - 301 * b for b in range(B)], np.int32)
    rows = [C.speech_like(int(n), C.SR) for n in lens]
    X, _ = C.padded(rows, np.nan)
    d_x = engine.to_device(X)

    def run():
        z, blocks = engine.loudness(d_x, C.SR, n_samples=lens, return_mean_square=True, want_blocks=True)[1:]
        work = engine.to_device(X)
        out, gains = engine.loudness_normalize(work, C.SR, -20.0, 0.9, n_samples=lens)
        y = out.to_host()
        work.free()
        return z, blocks, gains, y

    try:
        ref = run()
        # ... and the quiet run is right: two utterances against the oracle
        k = pkg('_hip').loudness_filter(C.SR)
        for b in (0, 11):
            wz, wJ, wP = O.mean_square(rows[b], C.SR, k)
            assert _bits64(ref[0][b]) == _bits64(wz) and tuple(ref[1][b]) == (wJ, wP)
            want = (np.float64(ref[2][b]) * rows[b].astype(np.float64)).astype(np.float32)
            assert np.array_equal(ref[3][b, :lens[b]].view(np.uint32), want.view(np.uint32))
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not (np.array_equal(_bits64(got[0]), _bits64(ref[0])) and np.array_equal(got[1], ref[1]) and
                        np.array_equal(_bits64(got[2]), _bits64(ref[2])) and np.array_equal(got[3].view(np.uint32), ref[3].view(np.uint32)))
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d_x.free()
