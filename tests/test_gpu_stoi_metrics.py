"""GPU: audio.metrics.stoi and datasets.statistics.collect_intelligibility.  At 22 050 Hz the figure is the oracle's
(tests/stoi_oracle.py) on what Engine.resample itself makes of the two signals, over the samples the resampler writes; at
10 000 Hz nothing is resampled.  collect_intelligibility runs on three short synthetic recordings written with save_wav; more
Griffin-Lim iterations must not lower its mean -- a sanity check, not a quality claim: no corpus is at hand."""
import numpy as np
import pytest

import stoi_cases as K
import stoi_oracle as S
from conftest import pkg

pytestmark = pytest.mark.gpu

VALUE_BOUND = 1e-9      # above every value bound of the rows of stoi_cases.bound_rows (tests/test_stoi_host.py asserts that)


def _pair(n, seed):
    x = K.speech(n=n, seed=seed, floor_db=-30.0)
    return x, K.degraded(x, 8, seed=20 + seed)


@pytest.mark.parametrize('extended', [False, True])
def test_at_another_rate_the_figure_is_the_oracle_on_the_resamplers_output(engine, extended):
    M, H = pkg('audio.metrics'), pkg('_hip')
    lens = np.array([30000, 26001], np.int32)
    ref, deg = np.full((2, 30000), np.nan, np.float32), np.full((2, 30000), np.nan, np.float32)     # the padding is poison
    for b, n in enumerate(lens):
        ref[b, :n], deg[b, :n] = _pair(int(n), b)
    got = M.stoi(ref, deg, 22050, extended=extended, n_samples=lens, engine=engine)
    assert got.shape == (2,) and got.dtype == np.float64
    ratio = 10000.0 / 22050.0
    for b, n in enumerate(lens):
        r10, d10 = engine.resample(ref[b, :n], ratio), engine.resample(deg[b, :n], ratio)
        valid = H.resampled_valid(int(n), ratio)
        o = S.stoi(r10.to_host()[:valid], d10.to_host()[:valid], extended)
        r10.free()
        d10.free()
        assert o['segments'] >= 5 and S.centred_ratios(o, extended) >= 1e-3
        assert abs(got[b] - o['value']) <= S.value_bound(o, extended) <= VALUE_BOUND, (b, got[b], o['value'])
        one = M.stoi(ref[b, :n], deg[b, :n], 22050, extended=extended, engine=engine)      # alone, no lengths: the same bits
        assert one.shape == (1,) and one.tobytes() == got[b:b + 1].tobytes()


def test_at_10_khz_nothing_is_resampled(engine):
    M = pkg('audio.metrics')
    ref, deg = K.row(('speech', 10))
    for extended in (False, True):
        got = M.stoi(ref, deg, 10000, extended=extended, engine=engine)
        o = K.oracle(('speech', 10), extended)
        assert abs(got[0] - o['value']) <= S.value_bound(o, extended)
    for rate in (2499, 40001):
        with pytest.raises(ValueError):
            M.stoi(ref, deg, rate, engine=engine)


def test_collect_intelligibility_on_three_short_recordings(engine, tmp_path):
    IO, ST = pkg('audio.io'), pkg('datasets.statistics')
    paths = []
    for k, n in enumerate((26000, 30000, 34000)):
        paths.append(str(tmp_path / ('rec%d.wav' % k)))
        IO.save_wav(paths[-1], np.asarray(K.speech(n=n, seed=k, floor_db=-30.0)), 22050)
    short = str(tmp_path / 'short.wav')
    IO.save_wav(short, np.asarray(K.speech(n=6000, floor_db=-30.0)), 22050)          # too short for a segment: NaN, not counted
    means = {}
    for iters in (1, 8):
        for extended in (False, True):
            res = ST.collect_intelligibility(paths + [short], iters, batch_size=3, seed=1, extended=extended, engine=engine)
            v = res['stoi']
            assert v.shape == (4,) and np.isfinite(v[:3]).all() and np.isnan(v[3]) and res['measured'] == 3
            assert (v[:3] > 0.0).all() and (v[:3] <= 1.0 + VALUE_BOUND).all()
            assert res['min'] == v[:3].min() and res['max'] == v[:3].max() and abs(res['mean'] - v[:3].mean()) < 1e-15
            assert abs(res['std'] - v[:3].std()) < 1e-15
            means[(iters, extended)] = res['mean']
            again = ST.collect_intelligibility(paths + [short], iters, batch_size=3, seed=1, extended=extended, engine=engine)
            assert again['stoi'].tobytes() == v.tobytes()
    print(means)
    for extended in (False, True):
        assert means[(8, extended)] >= means[(1, extended)] - VALUE_BOUND
