"""GPU: tts_true_peak and tts_limit (csrc/limiter.hip) against the numpy oracle of tests/limiter_oracle.py, bit for bit.

The shapes are the smallest at which the kernels can go wrong: lengths either side of a tile edge (2048 samples) and over two
tiles, look-aheads of 0, 1, 7 and the largest (1024, where the LDS of a workgroup is 147 KB and the halo is wider than a tile), a
row shorter than its look-ahead, peaks at both ends and either side of every tile edge, pairs closer than L and than 2 L, a
plateau, non-finite samples, and a ragged batch with NaN behind every length."""
import numpy as np
import pytest

import limiter_cases as C
import limiter_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

T = O.TILE
LENGTHS = (T - 1, T, T + 1, 2 * T + 3)


@pytest.fixture(scope='module')
def taps():
    return pkg('_hip').true_peak_filter()


def _limit(engine, x, L, oversample, n_samples=None, ceiling=C.CEILING):
    """-> (out (B, N) float32 host, stats (B,) records) of host rows"""
    d, stats = engine.limit(np.ascontiguousarray(x, np.float32), ceiling, L, oversample, n_samples=n_samples)
    out = d.to_host()
    d.free()
    return out, stats


def _assert_oracle(engine, taps, x, L, oversample, what, ceiling=C.CEILING):
    got, stats = _limit(engine, x[None], L, oversample, ceiling=ceiling)
    want, (over, limited, min_gain) = O.limit(x, taps, ceiling, L, oversample)
    diff = np.flatnonzero(C.bits(got[0]) != C.bits(want))
    assert diff.size == 0, (what, diff[:8], got[0][diff[:8]], want[diff[:8]])
    assert (int(stats['over'][0]), int(stats['limited'][0])) == (over, limited), (what, stats, over, limited)
    assert np.float64(stats['min_gain'][0]).view(np.uint64) == np.float64(min_gain).view(np.uint64), (what, stats, min_gain)
    finite = np.isfinite(want)
    assert np.all(np.abs(got[0][finite]) <= O.ceiling_float(ceiling))
    return want, (over, limited, min_gain)


@pytest.mark.parametrize('oversample', [1, 4])
@pytest.mark.parametrize('L', [0, 1, 7, O.MAX_LOOKAHEAD])
def test_the_limiter_is_the_oracle_bit_for_bit(engine, taps, L, oversample):
    for n in LENGTHS:
        _want, (over, limited, min_gain) = _assert_oracle(engine, taps, C.kitchen(n, L), L, oversample, (n, L, oversample))
        assert over > 0 and limited >= over and min_gain < 1.0


@pytest.mark.parametrize('oversample', [1, 4])
def test_rows_shorter_than_the_look_ahead_and_than_the_taps(engine, taps, oversample):
    for n, L in ((1, 0), (1, 7), (3, 7), (11, 110), (700, O.MAX_LOOKAHEAD)):
        x = C.speech_like(n, 1.6, seed=n + 17)
        x[0] = 0.9
        _assert_oracle(engine, taps, x, L, oversample, (n, L))


def test_a_row_under_the_ceiling_comes_back_as_its_bits(engine, taps):
    x = C.quiet(2 * T + 3)
    x[5] = -0.0
    for oversample in (1, 4):
        want, stats = _assert_oracle(engine, taps, x, 110, oversample, 'quiet')
        assert np.array_equal(C.bits(want), C.bits(x)) and stats == (0, 0, 1.0)
    # a ceiling exactly at the peak does not bind; one float below it does
    peak = float(np.abs(x).max())
    assert _assert_oracle(engine, taps, x, 7, 1, 'at the peak', ceiling=peak)[1] == (0, 0, 1.0)
    below = float(np.nextafter(np.float32(peak), np.float32(0)))
    assert _assert_oracle(engine, taps, x, 7, 1, 'below the peak', ceiling=below)[1][0] >= 1


@pytest.mark.parametrize('oversample', [1, 4])
def test_non_finite_samples_pass_through_and_reach_nothing_else(engine, taps, oversample):
    x = C.specials(T + 500)
    want, (over, limited, _g) = _assert_oracle(engine, taps, x, 7, oversample, 'specials')
    bad = ~np.isfinite(x)
    assert bad.sum() == 4 and np.array_equal(C.bits(want[bad]), C.bits(x[bad])) and over > 0
    assert C.bits(want[(T + 500) // 2]) == C.bits(np.float32(-0.0))


def test_a_ragged_batch_with_nan_padding_equals_its_rows_alone(engine, taps):
    L = 7
    rows = [C.kitchen(T + 1, L), C.quiet(900), C.kitchen(2 * T + 3, L), C.specials(T - 1), C.with_peaks(5, [0, 4])]
    X, lens = C.padded(rows, np.nan)
    for oversample in (1, 4):
        got, stats = _limit(engine, X, L, oversample, n_samples=lens)
        for b, r in enumerate(rows):
            want, (over, limited, min_gain) = O.limit(r, taps, C.CEILING, L, oversample)
            assert np.array_equal(C.bits(got[b, :len(r)]), C.bits(want)), (b, oversample)
            assert np.array_equal(C.bits(got[b, len(r):]), C.bits(X[b, len(r):])), b          # the poison is where it was
            assert (int(stats['over'][b]), int(stats['limited'][b]), float(stats['min_gain'][b])) == (over, limited, min_gain), b
            alone, stats1 = _limit(engine, r[None], L, oversample)
            assert np.array_equal(C.bits(alone[0]), C.bits(got[b, :len(r)])) and stats1[0] == stats[b], b
        assert tuple(stats[1]) == (0, 0, 1.0)


def test_more_rows_than_a_launch_takes(engine, taps):
    """65 rows: two launches; every row the bits of the oracle's"""
    L = 7
    rows = [C.with_peaks(300 + 7 * b, [b, 150, 150 + (b % 13)]) for b in range(65)]
    X, lens = C.padded(rows, np.nan)
    got, stats = _limit(engine, X, L, 4, n_samples=lens)
    for b in (0, 1, 31, 63, 64):
        want, st = O.limit(rows[b], taps, C.CEILING, L, 4)
        assert np.array_equal(C.bits(got[b, :lens[b]]), C.bits(want)) and tuple(stats[b]) == st, b


def test_the_true_peak_is_the_oracle_bit_for_bit(engine, taps):
    rows = [C.speech_like(n, 0.9) for n in LENGTHS] + [C.specials(T + 500), C.with_peaks(5, [0, 4]), np.zeros(40, np.float32),
                                                       np.full(3, np.nan, np.float32)]
    X, lens = C.padded(rows, np.nan)
    tp, sp = engine.true_peak(X, n_samples=lens, want_sample_peak=True)
    for b, r in enumerate(rows):
        wt, ws = O.true_peak(r, taps)
        assert np.float64(tp[b]).view(np.uint64) == np.float64(wt).view(np.uint64), (b, tp[b], wt)
        assert np.float64(sp[b]).view(np.uint64) == np.float64(ws).view(np.uint64), (b, sp[b], ws)
        assert tp[b] >= sp[b]
        one = engine.true_peak(r)
        assert one.shape == (1,) and one[0] == tp[b]
    assert tp[6] == 0.0 and tp[7] == 0.0 and sp[7] == 0.0
    # between the samples: sin(pi n / 2 + pi / 4) has a sample peak of 0.7071 and a true peak of 1 (its interior is held against
    # the interpolator's own error in tests/test_limiter_host.py; the edges ring)
    tone = np.sin(np.pi * np.arange(400) / 2 + np.pi / 4).astype(np.float32)
    t, s = engine.true_peak(tone, want_sample_peak=True)
    assert abs(s[0] - np.sqrt(0.5)) < 1e-6 and 0.99 < t[0] < 1.03


def test_the_profile_stage_and_its_launches(engine):
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        _limit(engine, C.kitchen(T + 1, 7)[None], 7, 4)
        ms, launches = engine.profile_get('limiter')
        assert launches == 4 and ms > 0                       # a fill, the records, the gains, the copy
        engine.profile_reset()
        engine.true_peak(C.quiet(900))
        assert engine.profile_get('limiter')[1] == 2          # a fill and the kernel
        engine.profile_reset()
        engine.true_peak(C.quiet(900), want_sample_peak=True)
        assert engine.profile_get('limiter')[1] == 3
    finally:
        engine.set_option('profile', 0)


def test_a_device_buffer_is_limited_in_place(engine, taps):
    x = C.kitchen(T + 1, 7)
    d = engine.to_device(x[None])
    try:
        out, stats = engine.limit(d, C.CEILING, 7, 1)
        assert out is d
        assert np.array_equal(C.bits(d.to_host()[0]), C.bits(O.limit(x, taps, C.CEILING, 7, 1)[0]))
    finally:
        d.free()
