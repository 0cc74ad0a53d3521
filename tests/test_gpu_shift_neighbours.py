"""tts_shift_magnitudes beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, and within the
oracle's bound, in the manner of tests/test_gpu_warp_neighbours.py -- a server shifts one batch while a second engine may be busy
on the same chip.  csrc/shift.hip: loads, stores and double arithmetic, no packed float32 arithmetic."""
import numpy as np
import pytest

import shift_cases as C
import shift_oracle as O
from conftest import pkg
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_shift_beside_gemm_launches_of_another_handle(engine, neighbour):
    H = pkg('_hip')
    eng2, launch = neighbour
    case = C.launch_seam()
    x = C.poisoned(C.batch(case['B'], 1025, case['T']), case['n_frames'])
    want = O.shift(x, case['segments'], case['n_frames'], 33)

    def run():
        rc, got, around = C.raw_shift(engine, H, x, case['n_frames'], case['segments'], 33, shift=1)
        assert rc == 0 and (around == C.NAN_PATTERN).all()
        return got

    ref = run()
    O.assert_holds(ref, want, 'quiet')
    bad = 0
    for _ in range(6):
        launch()
        got = run()
        eng2.synchronize()
        bad += not np.array_equal(got, ref)
    assert bad == 0, '%d of 6 results differ from the quiet run' % bad
