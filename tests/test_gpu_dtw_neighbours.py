"""tts_dtw beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_phase_init_neighbours.py -- an evaluation that measures mel-cepstral distortion runs the alignment of one batch
while a second engine may be busy on the same chip.  csrc/dtw.hip: double arithmetic, LDS and barriers, no packed float32
arithmetic and no atomics."""
import numpy as np
import pytest

import dtw_cases as K
import dtw_oracle as W
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_dtw_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    B, na, nb = 16, 150, 170
    pairs = [K.warped_pair(80 + p, na - p, nb - 2 * p, 13) for p in range(B)]
    A = np.zeros((B, na, 13), np.float32)
    Bm = np.zeros((B, nb, 13), np.float32)
    for p, (a, b) in enumerate(pairs):
        A[p, :a.shape[0]], Bm[p, :b.shape[0]] = a, b
    n_a = np.array([a.shape[0] for a, _ in pairs], np.int32)
    n_b = np.array([b.shape[0] for _, b in pairs], np.int32)
    d_a, d_b = engine.to_device(A), engine.to_device(Bm)
    run = lambda: engine.dtw(d_a, d_b, n_a=n_a, n_b=n_b, want_path=True)
    try:
        quiet = run()
        engine.synchronize()
        ref = [x.to_host().copy() for x in quiet]
        # ... and the quiet run is right: two pairs against the oracle
        for p in (0, 9):
            want = W.dtw_diagonals(*pairs[p])
            assert W.same_bits(ref[0][p], want[0]) and ref[1][p] == want[1]
            assert np.array_equal(ref[2][p], W.padded_path(want[2], na + nb - 1)), p
        bad = n = 0
        for _ in range(10):
            launch()
            outs = [run() for _ in range(2)]
            engine.synchronize()
            eng2.synchronize()
            for o in outs:
                n += 1
                bad += not (W.same_bits(o[0].to_host(), ref[0]) and np.array_equal(o[1].to_host(), ref[1]) and
                            np.array_equal(o[2].to_host(), ref[2]))
                for x in o:
                    x.free()
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
    finally:
        d_a.free()
        d_b.free()
