"""tts_f0 and tts_f0_compare beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the
manner of tests/test_gpu_dtw_neighbours.py -- an evaluation that measures F0 errors runs the tracker of one batch while a second
engine may be busy on the same chip.  csrc/f0.hip: double arithmetic, LDS, barriers and shuffles, no packed float32 arithmetic
and no atomics."""
import numpy as np
import pytest

import f0_cases as K
import f0_oracle as Y
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_f0_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    E = K.EVAL
    B, N = 16, 6000
    lens = np.array([N - 137 * p for p in range(B)], np.int32)
    X = np.zeros((B, N), np.float32)
    for b in range(B):
        X[b, :lens[b]] = K.tone(90.0 + 17.0 * b, int(lens[b]), seed=b) + 0.02 * K.content('noise', int(lens[b]), E['tau_max'], seed=b)
    d_x = engine.to_device(X)
    run = lambda: engine.f0(d_x, K.SR, E['hop'], window=E['W'], tau_min=E['tau_min'], tau_max=E['tau_max'], n_samples=lens,
                            want_aperiodicity=True)
    try:
        quiet = run()
        engine.synchronize()
        ref = [x.to_host().copy() for x in quiet]
        # ... and the quiet run is right: two utterances against the oracle
        for b in (0, 9):
            want = Y.f0(X[b:b + 1, :lens[b]], K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
            Tb = want[0].shape[1]
            assert Y.same_bits(ref[0][b, :Tb], want[0][0]) and Y.same_bits(ref[1][b, :Tb], want[1][0])
            assert (want[0][0] > 0).sum() >= Tb // 2
        # the comparison of the first half of the batch with the second, along diagonal paths
        Tf = ref[0].shape[1]
        path = np.stack([K.diagonal_path(Tf, Tf, 2 * Tf - 1)] * (B // 2))
        d_path = engine.to_device(path)
        d_f0 = quiet[0]
        half = (B // 2) * Tf * 4
        cmp_run = lambda: engine.f0_compare(_View(d_f0, 0, (B // 2, Tf)), _View(d_f0, half, (B // 2, Tf)), d_path)
        cq = cmp_run()
        engine.synchronize()
        cref = [x.to_host().copy() for x in cq]
        want = Y.compare(ref[0][0], ref[0][B // 2], path[0])
        assert np.array_equal(cref[0][0], want[0]) and Y.same_bits(cref[1][0, 0], want[1])
        bad = n = 0
        for _ in range(10):
            launch()
            outs = [run() for _ in range(2)]
            cmps = [cmp_run() for _ in range(2)]
            engine.synchronize()
            eng2.synchronize()
            for o, r in [(o, ref) for o in outs] + [(o, cref) for o in cmps]:
                n += 1
                bad += not all(Y.same_bits(x.to_host(), y) for x, y in zip(o, r))
                for x in o:
                    x.free()
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
        for x in tuple(cq) + (d_path,):
            x.free()
        for x in quiet:
            x.free()
    finally:
        d_x.free()


class _View(object):
    """a device buffer seen from a byte offset, for calls that take a data_ptr()"""

    def __init__(self, base, offset, shape):
        self.base, self.offset, self.shape = base, offset, shape

    def data_ptr(self):
        return self.base.data_ptr() + self.offset
