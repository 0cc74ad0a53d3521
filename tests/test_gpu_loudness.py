"""GPU: tts_loudness and tts_loudness_normalize (csrc/loudness.hip) against the numpy oracle of tests/loudness_oracle.py.

The measure -- the gated mean square and both block counts -- bit for bit (float64 compared as uint64) at the smallest shapes
where the kernels can go wrong: 22 050 Hz (unequal segments, 7 x 276 + 273) with no block, one block, a few, and both sides of a
segment edge; 16 000 Hz (equal segments) and 48 000 Hz; a ragged batch whose padding is NaN, each utterance the bits of its own
B = 1 call and of the batch in reversed order; the two gating signals; NaN samples inside and behind the counted blocks.

The normaliser: the gain against Python floats, every output sample the bits of float32(gain * float64(x)), the loudness of the
output, the peak ceiling, the bytes behind an utterance's end, and the utterances it must leave alone."""
import numpy as np
import pytest

import loudness_cases as C
import loudness_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu


def _coeffs(sr):
    return pkg('_hip').loudness_filter(sr)


def _measure(engine, x, sr, n_samples=None):
    """-> (z float64 (B,), blocks int32 (B, 2)) of host rows"""
    _lufs, z, blocks = engine.loudness(x, sr, n_samples=n_samples, return_mean_square=True, want_blocks=True)
    return z, blocks


def _same_z(got, want):
    got, want = np.float64(got), np.float64(want)
    return (np.isnan(got) and np.isnan(want)) or got.view(np.uint64) == want.view(np.uint64)


def _assert_oracle(engine, x, sr, what):
    z, blocks = _measure(engine, x[None], sr)
    wz, wJ, wP = O.mean_square(x, sr, _coeffs(sr))
    assert (int(blocks[0, 0]), int(blocks[0, 1])) == (wJ, wP), (what, blocks, wJ, wP)
    assert _same_z(z[0], wz), (what, float(z[0]), wz)
    return wz, wJ, wP


@pytest.mark.parametrize('sr,n', C.MEASURE)
def test_the_measure_is_the_oracle_bit_for_bit(engine, sr, n):
    assert engine.lib.tts_loudness_segment(sr) == O.segment(sr)
    z, J, passed = _assert_oracle(engine, C.speech_like(n, sr), sr, (sr, n))
    assert J == O.blocks(n, sr)
    if n == 4 * O.step(sr) - 1:
        assert (z, J, passed) == (0.0, 0, 0)          # no block: nothing is measured
    else:
        assert J >= 1 and passed >= 1 and -30.0 < O.lufs(z) < -18.0


def test_a_ragged_batch_with_nan_padding_equals_its_rows_alone_and_reversed(engine):
    rows = [C.speech_like(n, C.SR) for n in C.RAGGED]
    x, lens = C.padded(rows, np.nan)
    z, blocks = _measure(engine, x, C.SR, lens)
    k = _coeffs(C.SR)
    for b, r in enumerate(rows):
        wz, wJ, wP = O.mean_square(r, C.SR, k)
        assert _same_z(z[b], wz) and (int(blocks[b, 0]), int(blocks[b, 1])) == (wJ, wP), b
        z1, b1 = _measure(engine, r[None], C.SR)
        assert _same_z(z1[0], z[b]) and np.array_equal(b1[0], blocks[b]), b
    zr, br = _measure(engine, x[::-1].copy(), C.SR, lens[::-1].copy())
    assert all(_same_z(a, b) for a, b in zip(zr[::-1], z)) and np.array_equal(br[::-1], blocks)


@pytest.mark.parametrize('signal', ['relative_gate', 'absolute_gate'])
def test_the_gates(engine, signal):
    x = getattr(C, signal + '_signal')()
    z, J, passed = _assert_oracle(engine, x, 16000, signal)
    assert 0 < passed < J                                   # a gate dropped blocks
    plain = O.plain_mean_square(x, 16000, _coeffs(16000))
    assert abs(O.lufs(z) - O.lufs(plain)) < 1e-6
    assert round(float(O.lufs(z)), 2) == (-23.35 if signal == 'relative_gate' else -23.57)


def test_a_nan_reaches_its_own_utterance_only_and_only_from_a_counted_block(engine):
    s = O.step(C.SR)
    n = 6 * s + 100
    clean = C.speech_like(n, C.SR)
    inside, behind = clean.copy(), clean.copy()
    inside[2 * s + 11] = np.nan
    behind[6 * s + 50] = np.nan                             # behind the last block: counts for nothing
    inf = clean.copy()
    inf[5 * s] = np.inf
    z, blocks = _measure(engine, np.stack([clean, inside, behind, inf, clean]), C.SR)
    want = O.mean_square(clean, C.SR, _coeffs(C.SR))
    assert np.isfinite(want[0]) and want[0] > 0
    for b in (0, 2, 4):
        assert _same_z(z[b], want[0]) and tuple(blocks[b]) == want[1:], b
    for b, bad in ((1, inside), (3, inf)):
        assert np.isnan(z[b]) and tuple(blocks[b]) == (want[1], 0), b
        assert np.isnan(O.mean_square(bad, C.SR, _coeffs(C.SR))[0])
    lufs = engine.loudness(np.stack([clean, inside, np.zeros(n, np.float32)]), C.SR)
    assert np.isfinite(lufs[0]) and np.isnan(lufs[1]) and lufs[2] == -np.inf


def test_the_profile_stage(engine):
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        engine.loudness(C.speech_like(5 * O.step(C.SR), C.SR), C.SR)
        ms, launches = engine.profile_get('loudness')
        assert launches == 4 and ms > 0
    finally:
        engine.set_option('profile', 0)


# ---- the normaliser
def _normalize(engine, x, sr, target=-23.0, max_peak=1.0, n_samples=None):
    out, gains, z = engine.loudness_normalize(x, sr, target, max_peak, n_samples=n_samples, return_mean_square=True)
    y = out.to_host().copy()
    out.free()
    return y, gains, z


def test_the_gain_the_samples_and_the_loudness_of_the_output(engine):
    k = _coeffs(C.SR)
    rows = [C.speech_like(n, C.SR) for n in C.RAGGED[1:]]
    x, lens = C.padded(rows, np.nan)
    for target in (-23.0, -16.0):
        y, gains, z = _normalize(engine, x, C.SR, target, 1e6, lens)
        for b, r in enumerate(rows):
            wz = O.mean_square(r, C.SR, k)[0]
            assert _same_z(z[b], wz)
            want = np.sqrt(10.0 ** ((target + 0.691) / 10.0) / wz)
            assert abs(gains[b] - want) <= 1e-15 * want, (b, gains[b], want)
            out = (np.float64(gains[b]) * r.astype(np.float64)).astype(np.float32)
            assert np.array_equal(y[b, :len(r)].view(np.uint32), out.view(np.uint32)), b
            # the output reads the target, up to the float32 rounding of its samples
            again = O.lufs(O.mean_square(out, C.SR, k)[0])
            assert abs(again - target) < 1e-4, (b, again)
            assert abs(O.lufs(O.plain_mean_square(out, C.SR, k)) - target) < 1e-4
    back = engine.loudness(y, C.SR, n_samples=lens)
    assert np.all(np.abs(back - (-16.0)) < 1e-4)


def test_rows_behind_an_utterance_keep_their_bytes(engine):
    rows = [C.speech_like(n, C.SR) for n in C.RAGGED]
    x, lens = C.padded(rows, np.nan)
    rng = np.random.default_rng(7)
    tail = rng.integers(0, 2 ** 32, x.shape, dtype=np.uint64).astype(np.uint32)
    for b, n in enumerate(lens):
        x.view(np.uint32)[b, n:] = tail[b, n:]                # arbitrary bit patterns, NaNs among them
    y, gains, _z = _normalize(engine, x, C.SR, -20.0, 1e6, lens)
    for b, n in enumerate(lens):
        assert np.array_equal(y.view(np.uint32)[b, n:], x.view(np.uint32)[b, n:]), b
    assert gains[0] == 1.0 and np.all(gains[1:] != 1.0)


def test_the_peak_ceiling_binds(engine):
    x = np.stack([C.speech_like(C.RAGGED[2], C.SR), C.sine(C.SR, 0.52)[:C.RAGGED[2]] * np.float32(0.25)])
    x[1, 7] = np.inf                                         # a non-finite sample is no peak ...
    y, gains, z = _normalize(engine, x, C.SR, -3.0, 0.5)
    assert np.isnan(z[1]) and gains[1] == 1.0                # ... and its utterance is left alone
    assert np.array_equal(y[1].view(np.uint32), x[1].view(np.uint32))
    peak = O.finite_peak(x[0])
    free = np.sqrt(10.0 ** ((-3.0 + 0.691) / 10.0) / z[0])
    assert free > 0.5 / peak                                 # the ceiling binds
    assert gains[0] == np.float64(0.5) / np.float64(peak)
    assert np.abs(y[0]).max() <= 0.5
    # an Inf behind the last block: the measure does not see it, the peak skips it, the sample stays Inf
    x2 = x[:1].copy()
    x2[0, -3] = np.inf
    y2, g2, z2 = _normalize(engine, x2, C.SR, -3.0, 0.5)
    assert _same_z(z2[0], z[0]) and g2[0] == gains[0] and np.isinf(y2[0, -3])
    assert np.array_equal(np.delete(y2[0], len(y2[0]) - 3), np.delete(y[0], len(y[0]) - 3))


def test_silent_and_too_short_utterances_come_back_unchanged(engine):
    n = 5 * O.step(C.SR)
    short = C.speech_like(4 * O.step(C.SR) - 1, C.SR)
    quiet = (C.speech_like(n, C.SR) * np.float32(1e-5)).astype(np.float32)      # under the absolute gate
    x, lens = C.padded([np.zeros(n, np.float32), short, quiet], 0.0)
    y, gains, z = _normalize(engine, x, C.SR, -23.0, 1.0, lens)
    assert np.all(gains == 1.0) and np.all(z == 0.0)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
