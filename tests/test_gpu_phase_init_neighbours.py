"""The phase estimate beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner
of tests/test_gpu_resample_neighbours.py -- the pipelined tts_synthesize with "gl_init" = 1 puts exactly such neighbours side by
side (the encoder GEMMs of the next call beside the estimate of this one).  csrc/phase_init.hip: integer arithmetic, LDS
gathers and a few double operations per peak, no packed float32 arithmetic."""
import numpy as np
import pytest

import phase_cases as K
import phase_oracle as P
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def neighbour(hparams, weights):
    """A second handle whose only job is to keep MFMA GEMM waves on the chip."""
    eng2 = pkg().Engine(hparams)
    eng2.load_weights(weights)
    rng = np.random.default_rng(7)
    x = eng2.to_device(rng.standard_normal((9600, 256)).astype(np.float32))
    w = eng2.to_device(rng.standard_normal((256, 256)).astype(np.float32))
    c = eng2.empty((9600, 256))

    def launch(n=30):
        for _ in range(n):
            eng2._check(eng2.lib.tts_debug_gemm(eng2.handle, x.data_ptr(), w.data_ptr(), c.data_ptr(), 9600, 256, 256, 1, 150, 0))

    yield eng2, launch
    eng2.synchronize()
    for a in (x, w, c):
        a.free()
    eng2.close()


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
