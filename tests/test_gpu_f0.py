"""GPU: tts_f0 (csrc/f0.hip) against the numpy oracle of tests/f0_oracle.py, f0 and aperiodicity bit for bit (compared as uint32):
on the parameter grid of tests/f0_cases.py -- the smallest call, lags one short of a wave, a wave and one beyond it, the
evaluation's shape and the limits -- at lengths placed round a hop and a span, on every kind of content, at the three thresholds;
in a ragged batch whose padding is poison; across the cut of a launch; and the profile stage."""
import numpy as np
import pytest

import f0_cases as K
import f0_oracle as Y
from conftest import pkg

pytestmark = pytest.mark.gpu


def _run(engine, x, hop, W, lo, hi, thr, n_samples=None):
    """one call on host rows (B, N) -> host (f0, aperiodicity)"""
    f0, ap = engine.f0(x, K.SR, hop, window=W, tau_min=lo, tau_max=hi, threshold=thr, n_samples=n_samples, want_aperiodicity=True)
    out = f0.to_host().copy(), ap.to_host().copy()
    f0.free()
    ap.free()
    return out


def _assert_bits(got, want, what):
    for name, g, w in zip(('f0', 'aperiodicity'), got, want):
        g, w = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(w, np.float32)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        diff = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert diff.size == 0, (what, name, len(diff), diff[:4].tolist(), g[tuple(diff[0])], w[tuple(diff[0])])


@pytest.mark.parametrize('W,lo,hi,hop', K.GRID)
def test_the_grid_of_parameters_lengths_contents_and_thresholds(engine, W, lo, hi, hop):
    assert engine.lib.tts_f0_max_window() >= W and engine.lib.tts_f0_max_lag() >= hi
    voiced = 0
    for n in K.lengths(W, hi, hop):
        x = K.batch(n, hi)
        q, c_last = Y.normalised_difference(x, hop, W, hi)          # one oracle pass serves the three thresholds
        assert q.shape[1] == engine.lib.tts_f0_frames(n, hop)
        for thr in K.THRESHOLDS:
            want = Y.decide(q, c_last, K.SR, lo, hi, thr)
            _assert_bits(_run(engine, x, hop, W, lo, hi, thr), want, (n, thr))
            if thr == 0.0:
                assert not (want[0] > 0).any()
            if thr == float('inf'):
                finite = ~np.isnan(want[0])
                assert (want[0][finite] > 0).all()
            voiced += int((want[0] > 0).sum())
        # without an aperiodicity buffer: the same f0
        only = engine.f0(x, K.SR, hop, window=W, tau_min=lo, tau_max=hi, threshold=0.1)
        _assert_bits((only.to_host(), want[1]), (Y.decide(q, c_last, K.SR, lo, hi, 0.1)[0], want[1]), (n, 'f0 alone'))
        only.free()
    assert voiced > 0


@pytest.mark.parametrize('W,lo,hi,hop', [(63, 2, 63, 7), (1024, 44, 368, 275)])
def test_a_ragged_batch_equals_its_rows_alone(engine, W, lo, hi, hop):
    span = W + hi
    N = 3 * span + 5
    lens = [1, hop, 2 * span, N - 1, N]
    kinds = ['tone', 'noise', 'subharmonic', 'fading', 'integers']
    X = np.full((5, N), np.nan, np.float32)     # the padding is poison: never read
    rows = []
    for b, (n, kind) in enumerate(zip(lens, kinds)):
        rows.append(K.content(kind, n, hi, seed=b))
        X[b, :n] = rows[b]
    got = _run(engine, X, hop, W, lo, hi, 0.1, n_samples=np.array(lens, np.int32))
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    T = Y.frames(N, hop)
    for b, n in enumerate(lens):
        want = Y.f0(rows[b][None], K.SR, hop, W, lo, hi, 0.1)
        Tb = Y.frames(n, hop)
        alone = _run(engine, rows[b][None], hop, W, lo, hi, 0.1)      # N = its own length
        _assert_bits(alone, want, ('alone', b))
        _assert_bits((got[0][b, :Tb], got[1][b, :Tb]), (want[0][0], want[1][0]), ('batch', b))
        assert (got[0][b, Tb:] == 0).all() and (got[1][b, Tb:] == 0).all() and got[0].shape == (5, T)


@pytest.mark.parametrize('B', [65, 130])
def test_a_batch_beyond_one_launch(engine, B):
    W, lo, hi, hop = 63, 2, 63, 7
    N = 300
    rng = np.random.default_rng(B)
    lens = rng.integers(1, N + 1, B).astype(np.int32)
    lens[[0, 63, 64, B - 1]] = [N, 1, N - 1, 129]
    X = np.full((B, N), np.nan, np.float32)
    for b in range(B):
        X[b, :lens[b]] = K.content(K.CONTENTS[2 + b % 5], int(lens[b]), hi, seed=b)
    got = _run(engine, X, hop, W, lo, hi, 0.1, n_samples=lens)
    want = Y.f0(np.nan_to_num(X, nan=7.0), K.SR, hop, W, lo, hi, 0.1, n_samples=lens)   # (the oracle cuts the rows first)
    _assert_bits(got, want, B)


def test_a_nan_spoils_its_own_frames_only(engine):
    W, lo, hi, hop = 65, 3, 65, 30
    x = np.stack([K.content('tone', 900, hi, seed=s) for s in range(3)])
    clean = _run(engine, x, hop, W, lo, hi, 0.1)
    bad = x.copy()
    bad[1, 444] = np.nan
    got = _run(engine, bad, hop, W, lo, hi, 0.1)
    _assert_bits(got, Y.f0(bad, K.SR, hop, W, lo, hi, 0.1), 'nan')
    _assert_bits((got[0][[0, 2]], got[1][[0, 2]]), (clean[0][[0, 2]], clean[1][[0, 2]]), 'the other utterances')
    inside = np.array([Y.first_sample(t, hop, W, hi) <= 444 < Y.first_sample(t, hop, W, hi) + W + hi for t in range(got[0].shape[1])])
    assert np.array_equal(np.isnan(got[0][1]), inside) and np.array_equal(np.isnan(got[1][1]), inside) and inside.sum() >= 4


def test_refusals_and_the_profile_stage(engine):
    H = pkg('_hip')
    x = K.batch(500, 63)
    p = engine.to_device(x)
    out = engine.empty((x.shape[0], Y.frames(500, 7)))
    try:
        for W, lo, hi, word in ((2049, 2, 63, '2048'), (63, 2, 1025, '1024'), (63, 1, 63, '1024')):
            rc = engine.lib.tts_f0(engine.handle, p.data_ptr(), x.shape[0], 500, None, float(K.SR), 7, W, lo, hi, 0.1, out.data_ptr(), None)
            assert rc == H.TTS_ERR_UNSUPPORTED and word in engine.lib.tts_last_error(engine.handle).decode()
        with pytest.raises(ValueError):
            engine.f0(p, K.SR, 7, window=2049)
    finally:
        p.free()
        out.free()
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        got = _run(engine, x, 7, 63, 2, 63, 0.1)
        ms, launches = engine.profile_get('f0')
        assert launches == 1 and ms > 0
        big = np.concatenate([x] * 12)[:130]
        _run(engine, big, 7, 63, 2, 63, 0.1)
        assert engine.profile_get('f0')[1] == 1 + 3       # one launch per 64 utterances
    finally:
        engine.set_option('profile', 0)
    _assert_bits(got, Y.f0(x, K.SR, 7, 63, 2, 63, 0.1), 'after the refusals')
