"""tts_compress beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_equalizer_neighbours.py -- a server compresses one batch while a second engine may be busy on the same chip.
csrc/compressor.hip: double arithmetic and shuffles, 64 KB of LDS per workgroup, no packed float32 arithmetic."""
import numpy as np
import pytest

import compressor_cases as C
import compressor_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_compressor_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    B = 16
    lens = np.array([2 * O.TILE + 91 - 1201 * b for b in range(B)], np.int32)
    rows = [C.speech_like(int(n), amp=1.2) for n in lens]
    X, _ = C.padded(rows)
    p = C.params('speech')

    def run():
        work = engine.to_device(X)
        y, env = engine.compress(work, C.as_engine(p), n_samples=lens, envelope=True)
        got = y.to_host(), env.to_host()
        work.free()
        env.free()
        return got

    ref, ref_env = run()
    # ... and the quiet run is right: three utterances against the oracle
    for b in (0, 1, 11):
        w = O.compress(rows[b], p)
        ok, worst = C.held(ref[b, :lens[b]], w)
        assert ok and worst <= 1.0 and C.same_doubles(ref_env[b, :lens[b]], w.envelope), (b, worst)
    bad = 0
    for _ in range(6):
        launch()
        got, got_env = run()
        eng2.synchronize()
        same_env = all(C.same_doubles(got_env[b, :lens[b]], ref_env[b, :lens[b]]) for b in range(B))
        bad += not (np.array_equal(C.bits(got), C.bits(ref)) and same_env)
    assert bad == 0, '%d of 6 results differ from the quiet run' % bad
