"""GPU: the watermark through a telephone channel, every stage on the device -- embed, the look-ahead limiter, the resampler to
8000 Hz, the mu-law coder; the codes decoded on the host by table; then the resampler back and the detector
(``audio.metrics.detect_watermark`` does both).  The payload read is the payload written, the offset is the cut, zeta is above the
threshold, and a wrong key stays below it.  The strength (0.2 of the envelope) and the length (20 000 samples, under a second) are
those at which the numpy oracles of the same stages pass with more than twice the threshold (tests/test_watermark_host.py)."""
import numpy as np
import pytest

import watermark_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu


def test_the_mark_survives_the_limiter_8_khz_and_mu_law(engine):
    H, metrics = pkg('_hip'), pkg('audio.metrics')
    p = C.chain_params()
    assert engine.sampling_rate == C.CHAIN_SR
    marked = engine.watermark_embed(C.chain_signal(), C.as_engine(p))
    cut = engine.to_device(marked.to_host()[C.CHAIN_CUT:])
    marked.free()
    limited, stats = engine.limit(cut, C.CHAIN_CEILING, C.CHAIN_LOOKAHEAD, 4)
    assert stats['limited'].sum() > 0                                        # (the limiter does act on this row)
    down = engine.resample(limited, float(C.CHAIN_RATE) / C.CHAIN_SR)
    codes, _records = engine.encode(down, 'mulaw', dither=None)
    received = C.mulaw_decode(codes.to_host())
    for d in (cut, down, codes):
        d.free()
    assert received.dtype == np.float32 and abs(len(received) - (C.CHAIN_N - C.CHAIN_CUT) * C.CHAIN_RATE / C.CHAIN_SR) < 2
    found = metrics.detect_watermark(received, C.CHAIN_RATE, p.key, offsets=C.CHAIN_OFFSETS, engine=engine)
    print('zeta %.2f at offset %d, payload 0x%04X; the threshold is %.2f' % (found['zeta'], found['offset'], found['payload'], H.WM_THRESHOLD))
    assert found['payload'] == p.payload and found['offset'] == C.CHAIN_CUT
    assert found['zeta'] > H.WM_THRESHOLD and found['detected']
    wrong = metrics.detect_watermark(received, C.CHAIN_RATE, C.CHAIN_WRONG_KEY, offsets=C.CHAIN_OFFSETS, engine=engine)
    print('a wrong key: zeta %.2f' % wrong['zeta'])
    assert wrong['zeta'] < H.WM_THRESHOLD and not wrong['detected']
