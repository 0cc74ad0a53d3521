"""GPU: tts_mfcc (csrc/cepstrum.hip) against the float64 oracle of tests/cepstrum_oracle.py, element by element within
|out - y| <= 2^-24 |y| + 2^-40 sum_n |d[k][n]| |x[n]| (include/sstts_hip.h; tests/test_cepstrum_host.py shows what that bound
tells apart), ragged batches whose padding is never read, clipping, NaN containment and the Python facade."""
import numpy as np
import pytest

import cepstrum_oracle as C
from conftest import pkg

pytestmark = pytest.mark.gpu


def _rows(seed, B, T, n_mels):
    return np.random.default_rng(seed).random((B, T, n_mels)).astype(np.float32)


def _check(out, y, scale, what):
    out = np.asarray(out, np.float64)
    ok = ~np.isnan(y)
    excess = np.abs(out[ok] - y[ok]) / np.maximum(C.bound(y[ok], scale[ok]), 1e-300)
    print('{}: largest error / bound = {:.3f}'.format(what, excess.max() if excess.size else 0.0))
    assert C.within_bound(out, y, scale), what


@pytest.mark.parametrize('n_mels', [16, 80, 272, 1024])
@pytest.mark.parametrize('T', [1, 7, 130])
def test_within_the_bound_of_the_float64_oracle(engine, n_mels, T):
    x = _rows(n_mels + T, 2, T, n_mels)
    for n_mfcc in (1, 13, n_mels):
        out = engine.mfcc(x, n_mfcc)
        assert out.shape == (2, T, n_mfcc)
        y, scale = C.mfcc(x, n_mfcc)
        _check(out.to_host(), y, scale, 'n_mels {} T {} n_mfcc {}'.format(n_mels, T, n_mfcc))
        out.free()


def test_padded_rows_and_a_ragged_batch_whose_padding_is_poison(engine):
    B, T, n_mels, stride = 5, 37, 80, 91
    n_frames = np.array([37, 1, 20, 36, 9], np.int32)
    full = np.full((B, T, stride), np.nan, np.float32)          # columns n_mels .. stride - 1: never read
    full[:, :, :n_mels] = _rows(3, B, T, n_mels)
    for b in range(B):
        full[b, n_frames[b]:] = np.nan                          # rows behind n_frames: never read
    x = full[:, :, :n_mels]
    y, scale = C.mfcc(x, 14, n_frames)
    d_full = engine.to_device(full.reshape(B, T, stride))
    d_full.shape = (B, T, n_mels)
    got = engine.mfcc(d_full, 14, n_frames=n_frames, row_stride=stride).to_host()
    assert not np.isnan(got).any()
    _check(got, y, scale, 'ragged, padded rows')
    for b in range(B):
        assert (got[b, n_frames[b]:] == 0.0).all() and (np.signbit(got[b, n_frames[b]:]) == 0).all(), b
    # the host view a[:, :, :n_mels] of the padded array is uploaded as it is: the same bits
    again = engine.mfcc(x, 14, n_frames=n_frames, row_stride=stride).to_host()
    assert np.array_equal(again, got)
    # an utterance alone, with T = its own length: the same bits (nothing depends on the batch)
    for b in (0, 2, 4):
        n = int(n_frames[b])
        alone = engine.mfcc(np.ascontiguousarray(x[b:b + 1, :n]), 14).to_host()
        assert np.array_equal(alone[0], got[b, :n]), b
    d_full.free()


def test_more_utterances_than_one_launch_takes(engine):
    B, T, n_mels = 70, 3, 16
    x = _rows(4, B, T, n_mels)
    n_frames = (1 + np.arange(B) % T).astype(np.int32)
    got = engine.mfcc(x, 5, n_frames=n_frames).to_host()
    y, scale = C.mfcc(x, 5, n_frames)
    _check(got, y, scale, '70 utterances')
    assert (got[np.arange(T)[None, :] >= n_frames[:, None]] == 0.0).all()


def test_clip01_is_numpys_clip(engine):
    rng = np.random.default_rng(5)
    x = (3.0 * rng.random((2, 19, 80)) - 1.0).astype(np.float32)     # values in [-1, 2)
    x[0, 0, :4] = [-0.0, 0.0, 1.0, np.float32(1.0) + np.float32(2.0 ** -23)]
    x[1, 3, 2], x[1, 4, 2] = np.inf, -np.inf
    y, scale = C.mfcc(x, 13, clip01=True)
    assert np.isfinite(y).all()
    _check(engine.mfcc(x, 13, clip01=True).to_host(), y, scale, 'clipped')
    # ... and without the switch nothing is clipped (Inf - Inf sums are NaN in the oracle and in the kernel alike)
    y0, scale0 = C.mfcc(x[:1], 13)
    assert np.abs(y0 - y[:1]).max() > 0.1
    _check(engine.mfcc(x[:1], 13).to_host(), y0, scale0, 'unclipped')


def test_a_nan_stays_inside_its_frame(engine):
    x = _rows(6, 3, 11, 80)
    clean = engine.mfcc(x, 13, clip01=True).to_host()
    bad = x.copy()
    bad[1, 4, 79] = np.nan
    bad[2, 0, 0] = np.nan
    for clip in (False, True):
        ref = engine.mfcc(x, 13, clip01=clip).to_host()
        got = engine.mfcc(bad, 13, clip01=clip).to_host()
        hit = np.zeros((3, 11), bool)
        hit[1, 4] = hit[2, 0] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], ref[~hit])
    assert np.isfinite(clean).all()


def test_calculate_mfccs_and_the_profile_stage(engine):
    F = pkg('audio.features')
    rng = np.random.default_rng(7)
    mel_db = (100.0 * rng.random((80, 23)) - 100.0).astype(np.float32)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        got = F.calculate_mfccs(mel_db, 22050, 13, engine=engine)
        ms, n = engine.profile_get('mfcc')
        assert n == 1 and ms > 0
    finally:
        engine.set_option('profile', 0)
    assert got.shape == (13, 23) and got.dtype == np.float32
    y, scale = C.mfcc(mel_db.T[None], 13)
    _check(got.T[None], y, scale, 'calculate_mfccs')


def test_refusals_leave_the_handle_usable(engine):
    TE = pkg().TtsError
    x = _rows(8, 2, 5, 16)
    d = engine.to_device(x)
    out = engine.empty((2, 5, 4))
    lib, h = engine.lib, engine.handle
    INV = pkg('_hip').TTS_ERR_INVALID
    assert lib.tts_mfcc(h, None, 2, 5, 16, 16, None, 4, 0, out.ptr) == INV
    assert lib.tts_mfcc(h, d.ptr, 2, 5, 16, 15, None, 4, 0, out.ptr) == INV and b'row_stride' in lib.tts_last_error(h)
    assert lib.tts_mfcc(h, d.ptr, 2, 5, 16, 16, None, 17, 0, out.ptr) == INV
    y, scale = C.mfcc(x, 4)
    _check(engine.mfcc(d, 4).to_host(), y, scale, 'after refusals')
    assert TE is not None
    d.free()
    out.free()
