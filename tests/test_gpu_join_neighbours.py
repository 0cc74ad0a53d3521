"""tts_join beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone and as the oracle, in the
manner of tests/test_gpu_loudness_neighbours.py -- a server joins one batch while a second engine may be busy on the same chip.
csrc/join.hip: loads, stores and double arithmetic at the edges, no packed float32 arithmetic."""
import numpy as np
import pytest

import join_cases as C
import join_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_join_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    fade = 64
    pieces, groups = C.pieces_of(fade, 3)
    x = C.with_specials(C.batch(), pieces)
    N_out = C.odd_n_out(pieces, groups, fade)
    want, _n = O.join(x, pieces, groups, fade, N_out)
    d = engine.to_device(x)

    def run():
        rc, got, around = C.raw_join(engine, d, x.shape, pieces, groups, fade, N_out, shift=1)
        assert rc == 0 and (around == C.NAN_PATTERN).all()
        return got

    try:
        ref = run()
        C.assert_same(ref, want, 'quiet')
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not np.array_equal(got, ref)
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d.free()
