"""tts_equalize beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_limiter_neighbours.py -- a server equalises one batch while a second engine may be busy on the same chip.
csrc/equalizer.hip: double arithmetic and shuffles, 64 KB of LDS per workgroup, no packed float32 arithmetic."""
import numpy as np
import pytest

import equalizer_cases as C
import equalizer_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_equalizer_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    B = 16
    lens = np.array([2 * O.TILE + 91 - 1201 * b for b in range(B)], np.int32)
    rows = [C.speech_like(int(n)) for n in lens]
    X, _ = C.padded(rows)
    sos = C.cascade(8)

    def run():
        work = engine.to_device(X)
        y = engine.equalize(work, sos, n_samples=lens).to_host()
        work.free()
        return y

    ref = run()
    # ... and the quiet run is right: three utterances against the oracle
    for b in (0, 1, 11):
        assert C.same(ref[b, :lens[b]], O.equalize(rows[b], sos)), b
    bad = 0
    for _ in range(6):
        launch()
        got = run()
        eng2.synchronize()
        bad += not np.array_equal(C.bits(got), C.bits(ref))
    assert bad == 0, '%d of 6 results differ from the quiet run' % bad
