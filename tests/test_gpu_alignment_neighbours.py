"""tts_alignment_stats beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner
of tests/test_gpu_loudness_neighbours.py -- a server checks one batch's attention while a second engine may be busy on the same
chip.  csrc/alignment.hip: integer maxima, shuffles, integer atomics on the utterance's own counters and one chain of double
additions; nothing whose result could depend on what runs beside it."""
import numpy as np
import pytest

import alignment_cases as C
import alignment_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('Ts', [92, 257])
def test_alignment_stats_beside_gemm_launches_of_another_handle(engine, neighbour, Ts):
    eng2, launch = neighbour
    S, B = 40, 16
    ali = C.random_batch(S, B, Ts, tag=41)
    n_sent, n_steps = C.ragged_lengths(B, Ts, 3), C.ragged_lengths(B, S, 4)[::-1]
    d_ali = engine.to_device(ali)

    def run():
        return engine.alignment_stats(d_ali, n_sent=n_sent, n_steps=n_steps, want_durations=True, want_pos=True)

    def same(got, want):
        return (O.same_records(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and
                np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)))

    try:
        ref = run()
        assert same(ref, O.batch(ali, n_sent, n_steps))          # ... and the quiet run is right
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not same(got, ref)
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d_ali.free()
