"""GPU: tts_speech_interval against both ends of the end-of-speech oracle's interval (tests/join_oracle.py on tests/eos_oracle.py), exactly:
B = 3 utterances of T = 37 frames and F = 9 bins, rows 9 and 32 floats apart with the padding columns poisoned; no active frame,
a single one at 0 or at T - 1, NaN rows, +Inf and -Inf; and last_active is what tts_speech_frames reports."""
import numpy as np
import pytest

import join_oracle as O

pytestmark = pytest.mark.gpu

B, T, F = 3, 37, 9
THR = np.float32(0.5)


def batches():
    """name -> (B, T, F) float32 over a background below the threshold"""
    rng = np.random.default_rng(12)
    quiet = lambda: (rng.random((B, T, F)) * 0.4).astype(np.float32)
    out = {}
    x = quiet()
    out['none'] = x
    x = quiet()
    x[0, 0, 4] = 0.7                      # a single active frame at 0
    x[1, T - 1, 8] = np.nextafter(THR, np.float32(1))   # ... at T - 1, by the smallest value above the threshold
    x[2, 20, 0] = THR                     # equal to the threshold: not active
    out['single'] = x
    x = quiet()
    x[0, 5, :] = 0.9
    x[0, 5, 3] = np.nan                   # a row that holds a NaN is silent, whatever else it holds
    x[0, 9, 0] = 0.8
    x[0, 30, 8] = np.nan
    x[1, :, :] = np.nan                   # an utterance of NaN: no active frame
    x[2, 2, 1] = np.nan
    x[2, 3, 2] = 0.6
    x[2, 36, 7] = 0.6
    x[2, 36, 0] = np.nan
    x[2, 11, 5] = 0.51
    out['nan'] = x
    x = quiet()
    x[0, 4, 2] = np.inf                   # +Inf is active
    x[0, 31, :] = -np.inf                 # a row of -Inf is silent
    x[1, 7, :] = -np.inf
    x[1, 8, 8] = np.inf
    x[1, 9, 0] = -np.inf                  # -Inf beside values above the threshold: active
    x[1, 9, 1] = 0.9
    x[2, :, :] = -np.inf
    out['inf'] = x
    x = quiet() + np.float32(0.6)         # every frame active
    out['all'] = x
    return out


@pytest.mark.parametrize('row_stride', [9, 32])
def test_the_interval_is_the_references(engine, row_stride):
    for name, x in batches().items():
        want_first, want_last = O.speech_interval_batch(x, THR)
        if name == 'none':
            assert want_first.tolist() == want_last.tolist() == [-1, -1, -1]
        if name == 'single':
            assert (want_first.tolist(), want_last.tolist()) == ([0, T - 1, -1], [0, T - 1, -1])
        if name == 'nan':
            assert (want_first.tolist(), want_last.tolist()) == ([9, -1, 3], [9, -1, 11])
        if name == 'inf':
            assert (want_first.tolist(), want_last.tolist()) == ([4, 8, -1], [4, 9, -1])
        if name == 'all':
            assert (want_first.tolist(), want_last.tolist()) == ([0, 0, 0], [T - 1] * 3)
        for poison in ((np.nan, np.inf, 9.0) if row_stride > F else (0.0,)):
            full = np.full((B, T, row_stride), poison, np.float32)          # the padding columns are never read
            full[:, :, :F] = x
            d = engine.to_device(full)
            try:
                first, last = engine.speech_interval(d if row_stride == F else _view(d), THR, row_stride=row_stride)
                n_frames, last_frames = engine.speech_frames(d if row_stride == F else _view(d), THR, row_stride=row_stride)
                got = first.to_host(), last.to_host(), last_frames.to_host()
            finally:
                for a in (d, first, last, n_frames, last_frames):
                    a.free()
            assert got[0].dtype == np.int32 and got[0].tolist() == want_first.tolist(), (name, poison)
            assert got[1].tolist() == want_last.tolist() == got[2].tolist(), (name, poison)
    # a host array goes the same way (uploaded with its padding)
    x = batches()['nan']
    first, last = engine.speech_interval(x, THR, row_stride=row_stride)
    assert (first.to_host().tolist(), last.to_host().tolist()) == ([9, -1, 3], [9, -1, 11])


class _view(object):
    """a device buffer of (B, T, row_stride) floats seen as the (B, T, F) rows it holds"""

    def __init__(self, d):
        self.d, self.shape = d, (B, T, F)

    def data_ptr(self):
        return self.d.data_ptr()


def test_the_threshold_and_the_batch_do_not_reach_the_rule(engine):
    """an utterance's interval is the interval of the B = 1 call on its rows, at any threshold"""
    x = batches()['nan']
    for thr in (-1.0, 0.0, 0.5, 0.55, 0.85, 1.0, float('inf'), float('-inf')):
        want = O.speech_interval_batch(x, np.float32(thr))
        first, last = engine.speech_interval(x, thr)
        assert (first.to_host().tolist(), last.to_host().tolist()) == (want[0].tolist(), want[1].tolist()), thr
        for b in range(B):
            f1, l1 = engine.speech_interval(x[b:b + 1], thr)
            assert (f1.to_host()[0], l1.to_host()[0]) == (want[0][b], want[1][b]), (thr, b)
