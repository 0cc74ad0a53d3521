"""tts_watermark_embed and tts_watermark_detect beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits
as alone, in the manner of tests/test_gpu_compressor_neighbours.py -- a server marks one batch while a second engine may be busy
on the same chip.  csrc/watermark.hip: integer sums and a few double operations, up to 37 KB of LDS per workgroup, no packed float32
arithmetic."""
import numpy as np
import pytest

import watermark_cases as C
import watermark_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_watermark_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    B, D = 16, 40
    lens = np.array([2 * O.TILE + 91 - 301 * b for b in range(B)], np.int32)
    rows = [C.voiced(int(n)) for n in lens]
    X, _ = C.padded(rows)
    p = C.params('byte')

    def run():
        work = engine.to_device(X)
        y = engine.watermark_embed(work, C.as_engine(p), n_samples=lens)
        found = engine.watermark_detect(y, C.as_engine(p), offsets=D, n_samples=lens, want_scores=True, want_sums=True)
        got = (y.to_host(),) + found
        work.free()
        return got

    ref = run()
    # ... and the quiet run is right: three utterances against the oracle
    for b in (0, 1, 11):
        n = lens[b]
        assert np.array_equal(C.bits(ref[0][b, :n]), C.bits(O.embed(rows[b], p)[0])), b
        w = O.detect(ref[0][b, :n], p, D)
        assert (ref[1]['offset'][b], ref[1]['score'][b], ref[1]['energy'][b], ref[1]['payload'][b]) == (w.offset, w.score, w.energy, w.payload), b
        assert np.array_equal(ref[2][b], w.T) and np.array_equal(ref[3][b], w.S), b
    bad = 0
    for _ in range(6):
        launch()
        got = run()
        eng2.synchronize()
        bad += not all(a.tobytes() == r.tobytes() for a, r in zip(got, ref))
    assert bad == 0, '%d of 6 results differ from the quiet run' % bad
