"""tts_token_times beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_alignment_neighbours.py -- a server marks one batch's words while a second engine may be busy on the same chip.
csrc/token_times.hip: integer maxima and sums in LDS, barriers and shuffles; nothing whose result could depend on what runs
beside it.  One shape keeps its directions in LDS, the other in the workspace."""
import numpy as np
import pytest

import marks_cases as C
import marks_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('S,Ts', [(40, 92), (130, 300)])
def test_token_times_beside_gemm_launches_of_another_handle(engine, neighbour, S, Ts):
    eng2, launch = neighbour
    B = 16
    ali = C.batch('mixed', S, B, Ts, tag=41)
    n_sent, n_steps = C.ragged_lengths(B, Ts, 3), C.ragged_lengths(B, S, 4)[::-1]
    d_ali = engine.to_device(ali)

    def run():
        return engine.token_times(d_ali, n_sent=n_sent, n_steps=n_steps, max_jump=3, want_path=True)

    def same(got, want):
        return np.array_equal(got[0], want[0]) and O.same_records(got[1], want[1]) and np.array_equal(got[2], want[2])

    try:
        ref = run()
        assert same(ref, O.batch(ali, n_sent, n_steps, 3))       # ... and the quiet run is right
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not same(got, ref)
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d_ali.free()
