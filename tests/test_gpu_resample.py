"""GPU: tts_resample (csrc/resample.hip) against the float64 numpy oracle of resampy's windowed-sinc interpolator
(tests/resample_oracle.py: librosa 0.6 resample(..., res_type='kaiser_best'), reference audio/effects.py:9-43).  Every element is
held to
    |y - y64| <= 2^-24 |y64| + 2^-36 sum |w| |x|
-- the one rounding to float32, and the double accumulation and the table's libm with a hundredfold margin (resample_oracle.bound;
test_resample_host.py holds the bound to its model).

Shapes (tests/resample_cases.py): one ragged batch of lengths [1, 2, 63, 64, 700, 5000] at B = 6 and spread over B = 65 (more
than one launch's 64 utterances: groups of eight and single utterances), impulses in 700 samples, eight ratios; every output
buffer is pre-filled with NaN and every input carries NaN behind its utterance's length."""
import ctypes

import numpy as np
import pytest

import resample_cases as K
import resample_oracle as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(engine, x, rho, n_samples=None, N_out=None, fill=np.nan):
    """tts_resample into a buffer pre-filled with ``fill``; returns the host array (B, N_out)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, n = x.shape
    if N_out is None:
        N_out = R.resampled_length(max(n_samples) if n_samples is not None else n, rho)
    d_x = engine.to_device(x)
    d_out = engine.to_device(np.full((B, N_out), fill, np.float32))
    ns = None if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32)
    try:
        engine._check(engine.lib.tts_resample(engine.handle, d_x.data_ptr(), B, n,
                                              ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if ns is not None else None,
                                              float(rho), int(N_out), d_out.data_ptr()))
        return d_out.to_host()
    finally:
        d_x.free()
        d_out.free()


def hold(got, y64, sabs, label):
    """every element inside the bound; prints the worst ratio error / bound before it asserts"""
    assert got.shape == y64.shape and got.dtype == np.float32, label
    assert np.isfinite(got).all(), '{}: {} elements are not finite'.format(label, int((~np.isfinite(got)).sum()))
    err = np.abs(got.astype(np.float64) - y64)
    lim = R.bound(y64, sabs)
    worst = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print('{}: worst error / bound {:.3f}, max |err| {:.3e}'.format(label, worst, float(err.max()) if err.size else 0.0))
    bad = err > lim
    assert not bad.any(), '{}: {} of {} elements outside the bound, first at {}'.format(label, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def check_rows(got, rho, lengths, y64, sabs, label):
    N = got.shape[1]
    hold(got, K.fit(y64, N), K.fit(sabs, N), label)
    for b, n in enumerate(lengths):
        keep = min(R.resampled_valid(n, rho), N)
        tail = got[b, keep:]
        assert not tail.any() and not np.signbit(tail).any(), '{} b={}: the samples behind {} are not 0.0'.format(label, b, keep)


@pytest.mark.parametrize('rho', K.RATIOS, ids=K.RATIO_IDS)
def test_ragged_batch_against_the_oracle(engine, rho):
    """B = 6, N_out below, at and above ceil(5000 * rho); the same utterances spread over B = 65 give the same bits"""
    x = K.ragged_batch()
    y64, sabs = K.oracle('ragged', rho)
    full = None
    for N in K.n_out_choices(K.RAGGED_N, rho):
        got = run(engine, x, rho, K.RAGGED, N)
        check_rows(got, rho, K.RAGGED, y64, sabs, 'ragged rho={:.4f} N_out={}'.format(rho, N))
        if N == R.resampled_length(K.RAGGED_N, rho):
            full = got
    xs, ns = K.spread_batch()
    wide = run(engine, xs, rho, ns, full.shape[1])
    assert np.isfinite(wide).all()
    assert np.array_equal(bits(wide[K.SPREAD_AT]), bits(full)), 'an utterance changes with the batch around it'
    for b in range(K.SPREAD_B):
        keep = min(R.resampled_valid(int(ns[b]), rho), wide.shape[1])
        assert not wide[b, keep:].any()


@pytest.mark.parametrize('rho', K.RATIOS, ids=K.RATIO_IDS)
def test_impulses_hold_every_tap(engine, rho):
    """a single 1.0 at sample 0, 1, n / 2, n - 2, n - 1: output t is one tap of one phase, held to the bound on its own"""
    x = K.impulse_batch()
    y64, sabs = K.oracle('impulse', rho)
    got = run(engine, x, rho)
    check_rows(got, rho, [K.IMPULSE_N] * len(K.IMPULSE_AT), y64, sabs, 'impulse rho={:.4f}'.format(rho))
    assert np.abs(got).max() > 0.2     # (the main lobe: rolloff * min(1, rho) at its peak)


@pytest.mark.parametrize('rho', [0.5, 2.0 ** (-4.0 / 12.0), 1.0, 2.0 ** (3.0 / 12.0), 4.0], ids=['0.5', 'down4st', '1.0', 'up3st', '4.0'])
def test_a_nan_reaches_exactly_the_outputs_whose_window_covers_it(engine, rho):
    n, src = 700, 350
    x = K.ragged_batch()[4:5, :n].copy()
    clean = run(engine, x, rho)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[0, src] = bad
        got = run(engine, y, rho)
        want = np.zeros(got.shape[1], bool)
        cov = R.covers(n, rho, src)
        want[:cov.shape[0]] = cov
        assert want.sum() >= 100
        assert np.array_equal(~np.isfinite(got[0]), want), 'rho={} {}: {} outputs are not finite, the windows of {} cover it'.format(
            rho, bad, int((~np.isfinite(got[0])).sum()), int(want.sum()))
        assert np.array_equal(bits(got[0][~want]), bits(clean[0][~want]))


@pytest.mark.parametrize('rho', [0.5, 2.0 ** (3.0 / 12.0)], ids=['0.5', 'up3st'])
def test_an_utterance_does_not_depend_on_its_batch(engine, rho):
    x = K.ragged_batch()
    N = R.resampled_length(K.RAGGED_N, rho)
    whole = run(engine, x, rho, K.RAGGED, N)
    rev = run(engine, x[::-1], rho, K.RAGGED[::-1], N)
    assert np.array_equal(bits(rev), bits(whole[::-1]))
    for b, n in enumerate(K.RAGGED):
        one = run(engine, x[b:b + 1], rho, [n], N)
        assert np.array_equal(bits(one[0]), bits(whole[b])), b
    # eight copies take the kernel that applies a weight to eight utterances, one copy the single one: the same bits
    eight = run(engine, np.repeat(x[5:6], 8, axis=0), rho, [K.RAGGED[5]] * 8, N)
    for b in range(8):
        assert np.array_equal(bits(eight[b]), bits(whole[5])), b


def test_engine_resample_and_lengths(engine):
    H = pkg('_hip')
    x = K.ragged_batch()
    rho = 16000.0 / 22050.0
    d = engine.resample(x, rho, n_samples=K.RAGGED)
    assert d.shape == (len(K.RAGGED), R.resampled_length(K.RAGGED_N, rho))
    assert np.array_equal(bits(d.to_host()), bits(run(engine, x, rho, K.RAGGED)))
    d.free()
    one = engine.resample(x[5], 2.0)
    assert one.shape == (2 * K.RAGGED_N,)
    assert np.array_equal(bits(one.to_host()), bits(run(engine, x[5:6], 2.0)[0]))
    one.free()
    for n in (1, 2, 63, 700, 22050, 275000):
        for r in K.RATIOS:
            assert engine.resampled_length(n, r) == R.resampled_length(n, r) == H.resampled_length(n, r)
            assert H.resampled_valid(n, r) == R.resampled_valid(n, r)
    out = ctypes.c_int(-5)
    for n, r in [(0, 1.0), (5, float('nan')), (5, 0.2), (5, 4.5), (2 ** 30, 4.0)]:
        assert engine.lib.tts_resampled_length(n, r, ctypes.byref(out)) == H.TTS_ERR_INVALID and out.value == -5
    assert engine.lib.tts_resampled_length(5, 1.0, None) == H.TTS_ERR_INVALID


def test_refusals_leave_the_output_untouched(engine):
    H = pkg('_hip')
    B, n, N = 3, 100, 130
    d_x = engine.to_device(np.ones((B, n), np.float32))
    d_out = engine.to_device(np.full((B, N), -7.0, np.float32))
    I32 = ctypes.POINTER(ctypes.c_int32)

    def call(h=engine.handle, x=d_x.data_ptr(), B=B, n=n, ns=None, rho=1.3, N=N, out=d_out.data_ptr()):
        p = np.ascontiguousarray(ns, dtype=np.int32).ctypes.data_as(I32) if ns is not None else None
        return engine.lib.tts_resample(h, x, B, n, p, rho, N, out)

    try:
        assert call(h=None) == H.TTS_ERR_INVALID
        assert call(x=None) == H.TTS_ERR_INVALID and call(out=None) == H.TTS_ERR_INVALID
        for rho in (float('nan'), float('inf'), 0.0, 0.2, 4.5, -1.0):
            assert call(rho=rho) == H.TTS_ERR_INVALID
        assert call(B=0) == H.TTS_ERR_INVALID and call(n=0) == H.TTS_ERR_INVALID and call(N=0) == H.TTS_ERR_INVALID
        for bad in (0, -1, n + 1):
            assert call(ns=[n, bad, 1]) == H.TTS_ERR_INVALID
        engine.synchronize()
        assert np.array_equal(d_out.to_host(), np.full((B, N), -7.0, np.float32))
        assert call(ns=[n, 7, 1]) == H.TTS_OK
        got = d_out.to_host()
        assert np.isfinite(got).all() and not got[2, 1:].any() and not got[1, 9:].any()
        with pytest.raises(ValueError):
            engine.resample(np.ones((2, 10), np.float32), 5.0)
        with pytest.raises(ValueError):
            engine.resample(np.ones((2, 10), np.float32), 2.0, n_samples=[10, 11])
    finally:
        d_x.free()
        d_out.free()


def test_profile_stage_reports_its_launches(engine):
    """a launch per 64 utterances for their groups of eight and one for the utterances left over"""
    engine.set_option('profile', 1)
    try:
        counts = []
        for B in (6, 8, 13, 65):
            engine.profile_reset()
            run(engine, np.ones((B, 50), np.float32), 2.0)
            counts.append(engine.profile_get('resample')[1])
        assert counts == [1, 1, 2, 2]
        assert engine.profile_get('resample')[0] > 0
    finally:
        engine.set_option('profile', 0)
