"""The resampler beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_neighbours.py -- the pipelined tts_synthesize with a pitch puts exactly such neighbours side by side (the post-net
and encoder GEMMs of the next call beside the resampling of this one).  csrc/resample.hip: double FMAs and LDS reads, no packed
float32 arithmetic."""
import numpy as np
import pytest

import resample_cases as K
import resample_oracle as R
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('rho', [2.0 ** (-4.0 / 12.0), 2.0 ** (3.0 / 12.0)], ids=['down4st', 'up3st'])
def test_resample_beside_gemm_launches_of_another_handle(engine, neighbour, rho):
    eng2, launch = neighbour
    x = np.random.default_rng(11).standard_normal((16, 20000)).astype(np.float32)
    d_x = engine.to_device(x)
    run = lambda: engine.resample(d_x, rho)
    try:
        quiet = run()
        engine.synchronize()
        ref = quiet.to_host().copy()
        assert np.isfinite(ref).all()
        # ... and the quiet run is right: two utterances against the oracle
        for b in (0, 15):
            y64, sabs = R.resample(x[b].astype(np.float64), rho)
            assert (np.abs(ref[b].astype(np.float64) - y64) <= R.bound(y64, sabs)).all(), b
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
        d_x.free()
