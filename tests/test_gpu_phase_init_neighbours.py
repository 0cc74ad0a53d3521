"""The phase estimate beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner
of tests/test_gpu_resample_neighbours.py -- the pipelined tts_synthesize with "gl_init" = 1 puts exactly such neighbours side by
side (the encoder GEMMs of the next call beside the estimate of this one).  csrc/phase_init.hip: integer arithmetic, LDS
gathers and a few double operations per peak, no packed float32 arithmetic."""
import numpy as np
import pytest

import phase_cases as K
import phase_oracle as P
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_estimate_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    T = 100
    mag = np.stack([K.magnitudes(kind, 2048, T, seed=b) for b, kind in enumerate(['fixture', 'random', 'chirp', 'fixture'] * 4)])
    d_mag = engine.to_device(mag)
    run = lambda: engine.phase_estimate(d_mag, 2048, 275)
    try:
        quiet = run()
        engine.synchronize()
        ref = quiet.to_host().copy()
        # ... and the quiet run is right: two utterances against the oracle
        for b in (0, 2):
            assert np.array_equal(ref[b], P.phase_estimate(mag[b], 2048, 275)), b
        bad = n = 0
        for _ in range(10):
            launch()
            outs = [run() for _ in range(2)]
            engine.synchronize()
            eng2.synchronize()
            for o in outs:
                n += 1
                bad += not np.array_equal(o.to_host(), ref)
                o.free()
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
    finally:
        d_mag.free()
