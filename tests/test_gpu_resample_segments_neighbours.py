"""tts_resample_segments beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, and the
oracle's within its bound, in the manner of tests/test_gpu_warp_neighbours.py -- a server retimes one batch while a second engine
may be busy on the same chip.  csrc/resample_segments.hip: loads, stores, LDS and double arithmetic, no packed float32 arithmetic."""
import numpy as np
import pytest

import resample_oracle as R
import resample_segments_cases as C
from conftest import pkg
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_resample_segments_beside_gemm_launches_of_another_handle(engine, neighbour):
    H = pkg('_hip')
    eng2, launch = neighbour
    case, x = C.inputs('seam130')
    want = C.oracle('seam130', 3)
    N_out = want['y'].shape[1]

    def run():
        rc, got, around, _n = C.raw_call(engine, H, x, case['n_samples'], case['segments'], N_out, shift=1)
        assert rc == 0 and (around == C.NAN_PATTERN).all()
        return got

    ref = run()
    C.assert_matches(ref, want, 'quiet', R)
    bad = 0
    for _ in range(6):
        launch()
        got = run()
        eng2.synchronize()
        bad += not np.array_equal(got, ref)
    assert bad == 0, '%d of 6 results differ from the quiet run' % bad
