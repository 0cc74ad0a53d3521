"""STOI / ESTOI without a GPU: the library's host tables (tts_stoi_bands, tts_stoi_window) and the numpy oracle of
tests/stoi_oracle.py on the inputs of tests/stoi_cases.py -- what the figure does (1 for a copy, falling with the noise), the
special rows, the exact degenerate counts, and the value bound held from both sides: the oracle recomputed with a direct DFT in
np.longdouble stays within a quarter of it, the same pipeline with envelopes rounded to float32 breaks it.  The binding's
refusals are pinned on an Engine that has no handle."""
import numpy as np
import pytest

import stoi_cases as K
import stoi_oracle as S
from conftest import pkg
from host_checks import no_device_engine

BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219)]


def test_the_band_table_and_the_window():
    w, bands = S.tables()
    assert [tuple(r) for r in bands.tolist()] == BANDS
    want = np.hanning(258)[1:-1]
    assert w.shape == (256,) and (np.abs(w - want) <= np.spacing(want)).all()          # the last bit or one ulp
    formula = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(256) + 1) / 257)
    assert np.abs(w - formula).max() < 1e-15      # (two forms of one function: a few roundings of numbers near 0.5 apart)
    lib = pkg('').load_library()
    assert lib.tts_stoi_max_frames() == 65536
    assert [lib.tts_stoi_frames(n) for n in (1, 255, 256, 383, 384, 20000)] == [0, 0, 1, 1, 2, 155]


def test_the_speech_like_signal_keeps_76_of_155_frames():
    x = K.speech()
    E = S.energies(x)
    idx = S.kept_frames(E)
    assert (len(E), len(idx), S.segments(len(idx))) == (155, 76, 47)
    assert np.abs(E / (E.max() * 1e-4) - 1.0).min() > 0.05          # the frame nearest the threshold: 6 % away in energy


@pytest.mark.parametrize('extended', [False, True])
def test_a_copy_gives_one_and_noise_lowers_the_figure(extended):
    x = K.speech()
    assert abs(S.stoi(x, x, extended)['value'] - 1.0) <= 1e-12
    values = [S.stoi(x, K.degraded(x, snr), extended)['value'] for snr in K.SNRS]
    print(values)
    assert all(a > b for a, b in zip(values, values[1:])) and values[0] < 1.0 and values[-1] > 0.0


@pytest.mark.parametrize('extended', [False, True])
def test_the_special_rows(extended):
    x = K.speech()
    short = S.stoi(x[5000:5255], x[5000:5255], extended)
    assert (short['frames'], short['kept'], short['segments']) == (0, 0, 0) and np.isnan(short['value'])
    ref, deg = K.row(K.pattern_with_kept(29))
    o = S.stoi(ref, deg, extended)
    assert (o['kept'], o['segments'], o['degenerate']) == (29, 0, 0) and np.isnan(o['value'])
    zero = S.stoi(np.zeros(5000, np.float32), x[:5000], extended)
    assert (zero['frames'], zero['kept'], zero['segments']) == (38, 0, 0) and np.isnan(zero['value'])
    # a NaN in the reference drops its two frames and the rest is measured; in the degraded signal it spoils the value
    ref, deg = (a.copy() for a in K.row(('speech', 10)))
    base = S.stoi(ref, deg, extended)
    hole = ref.copy()
    at = 128 * int(base['index'][40]) + 200
    hole[at] = np.nan
    o = S.stoi(hole, deg, extended)
    assert o['kept'] == base['kept'] - 2 and np.isfinite(o['value'])
    deg[at] = np.nan
    assert np.isnan(S.stoi(ref, deg, extended)['value'])
    ref[at] = np.inf
    assert S.stoi(ref, deg, extended)['kept'] == 0


@pytest.mark.parametrize('extended', [False, True])
def test_the_degenerate_terms_where_they_are_exact(extended):
    ref, _ = K.row(K.pattern_with_kept(33))
    o = S.stoi(ref, np.zeros_like(ref), extended)              # a silent degraded signal: every envelope of it is 0.0
    assert o['segments'] == 4 and o['value'] == 0.0
    assert o['degenerate'] == o['segments'] * ((15 + 30) if extended else 15)
    # a band that is constant: the reference's band 3 the same in every frame
    base = S.stoi(ref, K.row(K.pattern_with_kept(33))[1], extended)
    X = base['X'].copy()
    X[3, :] = 0.25
    value, degenerate, _ = S.from_envelopes(X, base['Y'], extended)
    assert degenerate == o['segments'] * 1 and np.isfinite(value)   # a term of STOI, a row of ESTOI, per segment


def test_the_value_bound_from_both_sides():
    for key in K.bound_rows():
        ref, deg = K.row(key)
        for extended in (False, True):
            o = K.oracle(key, extended)
            assert o['degenerate'] == 0 and S.centred_ratios(o, extended) >= 1e-3, key
            bound = S.value_bound(o, extended)
            precise = S.stoi(ref, deg, extended, precise=True)
            rounded = S.stoi(ref, deg, extended, round_envelopes=np.float32)
            bx, by = S.envelope_bound(o)
            print(key[0], extended, o['kept'], 'bound %.3e precise %.3e float32 %.3e' % (bound, abs(precise['value'] - o['value']),
                                                                                        abs(rounded['value'] - o['value'])))
            assert abs(precise['value'] - o['value']) <= bound / 4, key
            assert (np.abs(precise['X'] - o['X']) <= bx / 4).all() and (np.abs(precise['Y'] - o['Y']) <= by / 4).all(), key
            assert abs(rounded['value'] - o['value']) > bound, key
            assert bound < 1e-9, key


def test_the_binding_refuses_before_the_library():
    eng = no_device_engine()
    x = np.zeros((2, 1000), np.float32)
    for call, text in ((lambda: eng.stoi(x, x[:, :900]), 'stoi: ref and deg must have one shape, got (2, 1000) and (2, 900)'),
                       (lambda: eng.stoi(x, x, extended=2), 'stoi: extended must be False / True (0 / 1), got 2'),
                       (lambda: eng.stoi(x, x, extended=1.0), 'stoi: extended must be False / True (0 / 1), got 1.0'),
                       (lambda: eng.stoi(x, x, n_samples=[1000]), 'n_samples: 2 integers are needed, got shape (1,) of int64'),
                       (lambda: eng.stoi(x, x, n_samples=[1000, 0]), 'n_samples[1] = 0 is not in 1 .. n = 1000'),
                       (lambda: eng.stoi(x, x, n_samples=[1000, 1001]), 'n_samples[1] = 1001 is not in 1 .. n = 1000'),
                       (lambda: eng.stoi(np.zeros((2, 3, 4), np.float32), x), 'stoi: one waveform (n,) or a batch (B, n) is needed, got shape (2, 3, 4)'),
                       (lambda: eng.stoi(np.zeros((1, 65536 * 128 + 256), np.float32), np.zeros((1, 65536 * 128 + 256), np.float32)),
                        'stoi: 65537 frames are more than 65536 (tts_stoi_max_frames)')):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == text
    M = pkg('audio.metrics')
    for rate in (2499, 40001, 22050.5, float('nan'), None):
        with pytest.raises(ValueError) as err:
            M.stoi(x, x, rate, engine=eng)
        assert str(err.value) == 'stoi: the sampling rate must be an integer in 2500 .. 40000, got {!r}'.format(rate)
    with pytest.raises(ValueError) as err:
        M.stoi(x, x[:, :5], 22050, engine=eng)
    assert str(err.value) == 'stoi: ref and deg must be waveforms (n,) or batches (B, n) of one shape, got (2, 1000) and (2, 5)'
