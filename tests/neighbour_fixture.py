"""The fixture of the tests that run a stage beside MFMA GEMM launches of ANOTHER handle (another set of streams): the test
modules import ``neighbour`` by name."""
import numpy as np
import pytest

from conftest import pkg


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
