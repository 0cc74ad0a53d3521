"""tts_encode beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same codes and records as alone, in the
manner of tests/test_gpu_limiter_neighbours.py -- a server encodes one batch while a second engine may be busy on the same chip.
csrc/encode.hip: double and 64-bit integer arithmetic, shuffles and integer atomics, no packed float32 arithmetic."""
import numpy as np
import pytest

import encode_cases as C
import encode_oracle as O
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_encode_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    B, N = 16, 3 * 4096 + 91
    lens = np.array([N - 301 * b for b in range(B)], np.int32)
    X = np.stack([C.speech_like(N, 1.05, seed=b) for b in range(B)])
    d_x = engine.to_device(X)

    def run():
        out = []
        for name in ('pcm16', 'mulaw'):
            codes, stats = engine.encode(d_x, name, seed=5, n_samples=lens)
            out += [codes.to_host(), stats]
            codes.free()
        return out

    try:
        ref = run()
        # ... and the quiet run is right
        for k, fmt in enumerate((O.S16, O.MULAW)):
            want, wst = O.encode(X, fmt, O.TPDF, 5, lens)
            assert C.same_bits(ref[2 * k], want) and C.same_records(ref[2 * k + 1], wst)
        bad = 0
        for _ in range(6):
            launch()
            got = run()
            eng2.synchronize()
            bad += not all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        assert bad == 0, '%d of 6 results differ from the quiet run' % bad
    finally:
        d_x.free()
