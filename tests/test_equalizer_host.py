"""CPU: the equaliser without a device.  (a) the segmented arithmetic of tests/equalizer_oracle.py (csrc/equalizer_plan.h restated)
against scipy's ``sosfilt`` over the whole signal, (b) the designs against ``scipy.signal.butter`` and against the same formulas in
``mpmath``, and their responses by properties, through Python and through the library, (c) what the 'telephony' profile is for, on
tones, and (d) the Python surface: ``equalizer_setting``, the SETTINGS row around a call on a library that records its calls,
the three older tables as they were, the helpers and the command line."""
import ctypes
import inspect

import numpy as np
import pytest

import equalizer_oracle as O
from conftest import pkg
from host_checks import no_device_engine

CAP = 2.0 ** -30          # of max |y|: a 64th of a float32 half-ulp at full scale, so the cut can never show in the output
N_NOISE = 100000
BUTTER = 1e-12            # per coefficient, relative: low-pass and high-pass sections against scipy.signal.butter
# Peak and shelf sections against the same formulas in mpmath (50 digits), the difference taken relative to the section's largest
# |coefficient| (a coefficient may pass through zero: b1 of a peak at f0 = sr / 4): 4 x the worst measured over GRID, 2.7e-15 -- a
# peak at 0.49 sr, Q 0.1, -40 dB, where tan(pi f0 / sr) = 31.8 magnifies the rounding of its argument 49 times
MPMATH = 4 * 2.7e-15
RATES = (8000, 22050, 48000, 192000)
RATIOS = (1e-4, 1e-3, 0.01, 0.1, 0.3, 0.45, 0.49)


def noise(n=N_NOISE, seed=1):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, n).astype(np.float32)


# ---------------------------------------------------------------------------------------------- (a) accuracy against scipy
def corners():
    cases = [('%s@%d' % (name, sr), O.profile(name, sr)) for name in sorted(O.PROFILES) for sr in (8000, 22050, 48000) if O.profile_fits(name, sr)]
    cases.append(('16th-order 20 Hz high-pass @192000', np.stack([O.design(O.HIGHPASS, 192000, 20.0, O.Q_BUTTER2)] * 8)))
    cases.append(('2nd-order 20 Hz high-pass @48000', O.design(O.HIGHPASS, 48000, 20.0, O.Q_BUTTER2)[None]))
    cases.append(('f0/sr = 1e-4 high-pass x 8 @8000', np.stack([O.design(O.HIGHPASS, 8000, O.F_MIN * 8000, O.Q_BUTTER2)] * 8)))
    cases.append(('low-pass at 0.49 sr', np.stack([O.design(O.LOWPASS, 22050, 0.49 * 22050, q) for q in O.Q_BUTTER4])))
    cases.append(('Q 30 peak +24 dB', O.design(O.PEAK, 22050, 1000.0, 30.0, 24.0)[None]))
    cases.append(('Q 30 peak -40 dB x 8', np.stack([O.design(O.PEAK, 22050, 500.0 * (s + 1), 30.0, -40.0) for s in range(8)])))
    cases.append(('Q 30 low-pass x 2 at 1e-3', np.stack([O.design(O.LOWPASS, 48000, 48.0, 30.0)] * 2)))
    cases.append(('shelves +24 / -40 dB', np.stack([O.design(O.LOWSHELF, 48000, 100.0, 0.1, 24.0), O.design(O.HIGHSHELF, 48000, 9000.0, 30.0, -40.0),
                                                   O.design(O.LOWSHELF, 48000, 300.0, 30.0, -40.0), O.design(O.HIGHSHELF, 48000, 4000.0, 0.1, 24.0)])))
    return cases


def test_the_cut_never_shows_against_sosfilt():
    from scipy.signal import sosfilt
    x = noise()
    cases = corners()
    assert len(cases) == 13 + 8
    worst = 0.0
    for name, sos in cases:
        y = O.equalize64(x, sos)
        ref = sosfilt(O.sosfilt_form(sos), x.astype(np.float64))
        diff = np.abs(y - ref).max() / np.abs(ref).max()
        print('%-40s %d sections  %.2e of max |y|' % (name, len(sos), diff))
        worst = max(worst, diff)
        assert np.all(np.isfinite(y)) and diff < CAP, (name, diff)
    print('worst %.2e, cap %.2e' % (worst, CAP))


def test_the_segmented_form_is_the_recurrence():
    """... and the plain recurrence, sample by sample, on lengths either side of every seam"""
    sos = O.profile('telephony', 22050)
    for n in (1, 255, 256, 257, 1000):
        x = noise(n, seed=n)
        y, ref = O.equalize64(x, sos), O.plain(x, sos)
        assert np.abs(y - ref).max() <= CAP * max(np.abs(ref).max(), 1e-30), n
    assert np.array_equal(O.equalize64(noise(256, 3), sos), O.plain(noise(256, 3), sos))       # one segment: no chain at all


# ---------------------------------------------------------------------------------------------- (b) the designs
def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


def test_low_and_high_pass_sections_are_scipys_butterworth():
    from scipy.signal import butter
    H = pkg('_hip')
    worst = 0.0
    for sr in RATES:
        for ratio in RATIOS:
            f0 = ratio * sr
            for kind, btype in ((O.LOWPASS, 'lowpass'), (O.HIGHPASS, 'highpass')):
                ref = butter(2, f0, btype, fs=sr, output='sos')[0]
                for got in (O.design(kind, sr, f0, O.Q_BUTTER2), np.array(H.equalizer_design(kind, sr, f0, H.EQ_Q_BUTTER2))):
                    d = rel(got, ref[[0, 1, 2, 4, 5]]).max()
                    worst = max(worst, d)
                    assert d < BUTTER, (sr, ratio, btype, d)
                # two sections: scipy keeps the whole gain in its first section
                ref = butter(4, f0, btype, fs=sr, output='sos')
                got = np.stack([O.design(kind, sr, f0, q) for q in O.Q_BUTTER4])
                d = max(rel(got[:, 3:], ref[:, 4:]).max(), rel(got[0, 0] * got[1, 0], ref[0, 0] * ref[1, 0]))
                worst = max(worst, d)
                assert d < BUTTER, (sr, ratio, btype, d)
                shape = (1.0, 2.0, 1.0) if kind == O.LOWPASS else (1.0, -2.0, 1.0)
                assert np.array_equal(got[:, :3] / got[:, :1], [shape, shape]) and np.array_equal(ref[1, :3], shape)
    print('worst difference from butter: %.2e' % worst)


GRID = [(kind, sr, ratio * sr, q, g) for kind in (O.PEAK, O.LOWSHELF, O.HIGHSHELF) for sr in (8000, 22050, 192000) for ratio in (1e-4, 0.01, 0.25, 0.3, 0.49)
        for q in (0.1, O.Q_BUTTER2, 30.0) for g in (-40.0, -3.0, 2.0, 24.0)]


def mp_design(kind, sr, f0, q, g):
    import mpmath as mp
    mp.mp.dps = 50
    f0, q, g = mp.mpf(f0), mp.mpf(q), mp.mpf(g)
    K = mp.tan(mp.pi * f0 / sr)
    KK, KQ, A = K * K, K / q, mp.mpf(10) ** (g / 40)
    if kind == O.PEAK:
        b, a = (1 + KQ * A + KK, 2 * (KK - 1), 1 - KQ * A + KK), (1 + KQ / A + KK, 2 * (KK - 1), 1 - KQ / A + KK)
    else:
        s = mp.sqrt(A) * KQ
        lift, rest = (1 + A * KK + s, 2 * (A * KK - 1), 1 + A * KK - s), (A + KK + s, 2 * (KK - A), A + KK - s)
        b, a = (tuple(A * v for v in lift), rest) if kind == O.LOWSHELF else (tuple(A * v for v in rest), lift)
    return [b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]]


def test_peak_and_shelf_sections_are_their_formulas_in_mpmath():
    H = pkg('_hip')
    lib = H.load_library()
    five = (ctypes.c_double * 5)()
    worst = 0.0
    for kind, sr, f0, q, g in GRID:
        ref = mp_design(kind, sr, f0, q, g)
        scale = max(abs(v) for v in ref)
        assert lib.tts_equalizer_design(kind, sr, f0, q, g, five) == H.TTS_OK
        for got in (O.design(kind, sr, f0, q, g), H.equalizer_design(kind, sr, f0, q, g), five[:]):
            d = max(float(abs(v - r) / scale) for v, r in zip(got, ref))
            worst = max(worst, d)
            assert d <= MPMATH, (kind, sr, f0, q, g, d)
    print('worst difference from mpmath: %.2e of the largest coefficient' % worst)


def test_peaks_and_shelves_by_their_responses():
    db = lambda v: 20.0 * np.log10(v)
    for sr in (8000, 22050, 48000):
        for f0 in (0.001 * sr, 0.05 * sr, 0.3 * sr):
            for q in (0.3, O.Q_BUTTER2, 5.0):
                for g in (-40.0, -6.0, 3.0, 24.0):
                    peak = O.design(O.PEAK, sr, f0, q, g)
                    assert abs(db(O.response(peak, f0, sr)) - g) < 1e-8
                    assert abs(db(O.response(peak, 0.0, sr))) < 1e-9 and abs(db(O.response(peak, sr / 2.0, sr))) < 1e-9
                    low, high = O.design(O.LOWSHELF, sr, f0, q, g), O.design(O.HIGHSHELF, sr, f0, q, g)
                    for shelf, lifted, flat in ((low, 0.0, sr / 2.0), (high, sr / 2.0, 0.0)):
                        assert abs(db(O.response(shelf, f0, sr)) - g / 2.0) < 1e-8
                        assert abs(db(O.response(shelf, lifted, sr)) - g) < 1e-8 and abs(db(O.response(shelf, flat, sr))) < 1e-8
                    # ... and tends there: a decade and a half either side of a low corner
                    if f0 / sr < 0.01 and q == O.Q_BUTTER2:
                        assert abs(db(O.response(low, f0 / 30.0, sr)) - g) < 0.02 * abs(g) and abs(db(O.response(low, f0 * 30.0, sr))) < 0.02 * abs(g)
                        assert abs(db(O.response(high, f0 * 30.0, sr)) - g) < 0.02 * abs(g) and abs(db(O.response(high, f0 / 30.0, sr))) < 0.02 * abs(g)


def test_the_library_designs_and_profiles_are_pythons():
    H = pkg('_hip')
    lib = H.load_library()
    from conftest import ROOT
    import os
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in ('tts_equalize', 'tts_equalizer_design', 'tts_equalizer_profile', 'tts_equalizer_max_sections', 'tts_set_equalizer'):
        assert name in H.exported_symbols() and getattr(lib, name) is not None and 'int {}('.format(name) in header
    assert lib.tts_equalizer_max_sections() == O.MAX_SECTIONS == H.EQ_MAX_SECTIONS
    assert (H.EQ_SR_MIN, H.EQ_SR_MAX, H.EQ_F_MIN, H.EQ_F_MAX, H.EQ_Q_MIN, H.EQ_Q_MAX, H.EQ_GAIN_MIN, H.EQ_GAIN_MAX) == \
        (O.SR_MIN, O.SR_MAX, O.F_MIN, O.F_MAX, O.Q_MIN, O.Q_MAX, O.GAIN_MIN, O.GAIN_MAX)
    assert H.EQ_KINDS == O.KINDS and sorted(H.EQ_PROFILES) == sorted(O.PROFILES)
    five, forty, n = (ctypes.c_double * 5)(), (ctypes.c_double * 40)(), ctypes.c_int(0)
    for sr in RATES:
        for ratio in RATIOS:
            for kind in (O.LOWPASS, O.HIGHPASS):
                for q in O.Q_BUTTER4 + (O.Q_BUTTER2,):
                    assert lib.tts_equalizer_design(kind, sr, ratio * sr, q, 0.0, five) == H.TTS_OK
                    assert rel(five[:], H.equalizer_design(kind, sr, ratio * sr, q)).max() < BUTTER
    for name in O.PROFILES:
        assert [(H.EQ_KINDS[k], f0, q, g) for k, f0, q, g in H.EQ_PROFILES[name]] == list(O.PROFILES[name])
        for sr in (8000, 16000, 22050, 44100, 48000, 192000):
            rc = lib.tts_equalizer_profile(name.encode(), sr, forty, ctypes.byref(n))
            if not O.profile_fits(name, sr):
                assert rc == H.TTS_ERR_UNSUPPORTED and "'{}'".format(name).encode() in lib.tts_last_error(None)
                with pytest.raises(ValueError, match=name):
                    H.equalizer_profile(name, sr)
                continue
            want = H.equalizer_profile(name, sr)
            assert rc == H.TTS_OK and n.value == len(want) == len(O.PROFILES[name])
            got = np.array(forty[:5 * n.value]).reshape(-1, 5)
            assert np.abs(got - want).max() <= MPMATH * np.abs(want).max() and np.abs(want - O.profile(name, sr)).max() <= MPMATH * np.abs(want).max()
    assert lib.tts_equalizer_profile(b'telephony', 7999, forty, ctypes.byref(n)) == H.TTS_ERR_UNSUPPORTED
    assert lib.tts_equalizer_profile(b'phone', 22050, forty, ctypes.byref(n)) == H.TTS_ERR_INVALID
    assert lib.tts_equalizer_design(0, 22050, 1000.0, 0.7, 0.0, None) == H.TTS_ERR_INVALID


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal is made on the arguments alone, ahead of the handle, in the order the header lists them.  The pointers are
    never dereferenced."""
    H = pkg('_hip')
    lib = H.load_library()
    INV = H.TTS_ERR_INVALID
    p, q = 4096, 1 << 20   # aligned non-NULL addresses

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    def arr(values):
        a = np.ascontiguousarray(values, np.float64)
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a

    def i32(values):
        a = np.ascontiguousarray(values, np.int32)
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), a

    sos, _k = arr(O.profile('telephony', 22050))
    nan_k, _k1 = arr([[1.0, 0.0, float('nan'), 0.0, 0.0]])
    unstable, _k2 = arr([[1.0, 0.0, 0.0, 0.0, 1.0]])
    good, _k3 = i32([5000, 1, 275])
    bad, _k4 = i32([5000, 0, 275])
    assert lib.tts_equalize(None, p, q, 3, 5000, good, sos, 4) == INV            # a good call: only the handle is missing
    for args, text in (
            ((None, q, 3, 5000, None, sos, 4), 'equalize: a NULL pointer'),
            ((p, None, 3, 5000, None, sos, 4), 'equalize: a NULL pointer'),
            ((p, q, 3, 5000, None, None, 4), 'equalize: a NULL pointer'),
            ((p, q, 0, 5000, None, sos, 0), 'equalize: need B, N >= 1'),
            ((p, q, 3, 0, None, sos, 0), 'equalize: need B, N >= 1'),
            ((p + 2, q, 3, 5000, bad, sos, 0), 'equalize: n_samples[1] = 0 is not in 1 .. N = 5000'),
            ((p + 2, q, 3, 5000, None, nan_k, 0), 'equalize: n_sections = 0 is not in 1 .. EQ_MAX_SECTIONS = 8'),
            ((p + 2, q, 3, 5000, None, nan_k, 9), 'equalize: n_sections = 9 is not in 1 .. EQ_MAX_SECTIONS = 8'),
            ((p + 2, q, 3, 5000, None, nan_k, 1), 'equalize: coefficient 2 of section 0 is not finite'),
            ((p + 2, q, 3, 5000, None, unstable, 1), 'equalize: section 0 is not stable'),
            ((p + 2, p + 6, 3, 5000, None, sos, 4), 'equalize: wav and out must be 4-byte aligned'),
            ((p, q + 1, 3, 5000, None, sos, 4), 'equalize: wav and out must be 4-byte aligned'),
            ((p, p + 4, 3, 5000, None, sos, 4), 'equalize: out overlaps wav without being equal to it'),
            ((p + 4 * 3 * 5000 - 4, p, 3, 5000, None, sos, 4), 'equalize: out overlaps wav without being equal to it')):
        assert lib.tts_equalize(None, *args) == INV and why().startswith(text), (args, why())
    assert lib.tts_equalize(None, p, p, 3, 5000, None, sos, 4) == INV and lib.tts_equalize(None, p, p + 4 * 3 * 5000, 3, 5000, None, sos, 4) == INV
    assert lib.tts_set_equalizer(None, 1, sos, 4) == INV and lib.tts_set_equalizer(None, 0, None, 0) == INV


# ---------------------------------------------------------------------------------------------- (c) what it is for
def test_telephony_keeps_the_voice_band_and_drops_what_is_outside():
    """tones of amplitude 1 at 22050 Hz through the oracle: the amplitude over the last 2048 of 8192 samples, by a least-squares
    fit of the tone.  1 / (1 + r ** 8) with the tan-warped ratios r of about 2.9 to 3.0 is -37 dB."""
    sr, n = 22050, 8192
    sos = O.profile('telephony', sr)
    t = np.arange(n, dtype=np.float64)

    def level(f):
        y = O.equalize(np.sin(2 * np.pi * f * t / sr).astype(np.float32), sos).astype(np.float64)[-2048:]
        basis = np.stack([np.sin(2 * np.pi * f * t[-2048:] / sr), np.cos(2 * np.pi * f * t[-2048:] / sr)], 1)
        a, b = np.linalg.lstsq(basis, y, rcond=None)[0]
        return 20.0 * np.log10(np.hypot(a, b))

    levels = {f: level(f) for f in (1000.0, 100.0, 7000.0)}
    print(levels)
    assert abs(levels[1000.0]) < 0.1
    assert levels[100.0] < -30.0 and levels[7000.0] < -30.0
    for f in levels:
        assert abs(levels[f] - 20.0 * np.log10(O.response(sos, f, sr))) < 0.05


# ---------------------------------------------------------------------------------------------- (d) the Python surface
def test_equalizer_setting_accepts_and_refuses_as_documented():
    H = pkg('_hip')
    S = H.equalizer_setting
    assert S(None) is None
    assert S('telephony') == ('profile', 'telephony') and all(S(name) == ('profile', name) for name in H.EQ_PROFILES)
    assert S([('highpass', 120)]) == ('design', (('highpass', 120.0, H.EQ_Q_BUTTER2, 0.0),))
    assert S([('peak', 3000, 1.0, 3), (4, 6000.0, None, 2.0)]) == ('design', (('peak', 3000.0, 1.0, 3.0), ('highshelf', 6000.0, H.EQ_Q_BUTTER2, 2.0)))
    sos = O.profile('warm', 22050)
    assert S(sos) == ('sos', tuple(tuple(float(v) for v in row) for row in sos)) == S(sos.tolist())
    for checked in (S('bright'), S([('peak', 3000, 1.0, 3)]), S(sos)):
        assert S(checked) == checked                                      # a checked value is taken as it is
        assert hash(checked) is not None
    for bad in ('phone', '', 5, 0.5, True, [], [('peak',)], [('notch', 100.0)], [('peak', -1.0)], [('peak', float('nan'))], [('peak', 'a')],
                [('peak', 100.0, 0.05)], [('peak', 100.0, 31.0)], [('peak', 100.0, 1.0, 25.0)], [('lowshelf', 100.0, 1.0, -41.0)],
                [('peak', 100.0, 1.0, 0.0, 7)], [('highpass', 100.0)] * 9, np.zeros((2, 4)), np.zeros((9, 5)), np.zeros((0, 5)), np.zeros(5),
                [[1.0, 0.0, 0.0, 0.0, float('nan')]], [[1.0, 0.0, 0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0, 2.0, 0.99]], [[1.0, 0.0, 0.0, -1.5, 0.5]]):
        with pytest.raises(ValueError):
            S(bad)
    # what depends on the rate is refused where the rate is known
    assert H.equalizer_sections(S('telephony'), 8000).shape == (4, 5)
    np.testing.assert_array_equal(H.equalizer_sections(S(sos), 8000), sos)
    for setting, sr in ((S('bright'), 8000), (S([('lowpass', 11000.0)]), 22050), (S([('highpass', 1.0)]), 22050), (S('rumble'), 200000), (S('rumble'), 7999)):
        with pytest.raises(ValueError):
            H.equalizer_sections(setting, sr)
    with pytest.raises(ValueError, match="'bright'"):
        H.equalizer_profile('bright', 8000)
    # the entry points refuse before they touch a handle
    eng = no_device_engine()
    X = np.zeros((2, 5000), np.float32)
    for call in (lambda: eng.equalize(X, None), lambda: eng.equalize(X, 'phone'), lambda: eng.equalize(np.zeros((1, 2, 3), np.float32), 'warm'),
                 lambda: eng.equalize(X, 'warm', n_samples=[5000, 5001]), lambda: eng.equalize(X, 'warm', out=X),
                 lambda: eng.set_equalizer('phone'), lambda: eng.set_equalizer([('lowpass', 11025.0)]),
                 lambda: pkg('audio.effects').equalize(X, 8000, 'bright', engine=eng), lambda: pkg('audio.effects').equalize(X, 22050, None, engine=eng)):
        with pytest.raises(ValueError):
            call()
    ids = np.zeros((1, 4), np.int32)
    for bad in ('phone', 0.5, [('notch', 100.0)], np.zeros((2, 4))):
        with pytest.raises(ValueError):
            eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, equalizer=bad)
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, equalizer=bad)


def test_the_equalizer_row_is_the_last_of_the_settings_table():
    H = pkg('_hip')
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[-1]                                      # the last row: set last, put back first
    assert (row.keyword, row.mirror, row.initial, row.host_only) == ('equalizer', '_equalizer', None, False) and row.check is H.equalizer_setting
    assert keys[-2:] == ['compressor', 'equalizer']
    assert no_device_engine()._equalizer is None


def test_the_keyword_is_set_last_and_put_back_first():
    """the last row of SETTINGS around a call, on a library that records its calls (as tests/test_settings_host.py holds the first
    seven rows and tests/test_limiter_host.py the eighth)"""
    import test_settings_host as S
    H = pkg('_hip')
    eng = no_device_engine()
    eng.lib = S.RecordingLibrary()
    eng.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    eng._staging, eng._host_shapes, eng._host_out_shapes = {}, {}, {}
    on, off = ('tts_set_equalizer', (1, 4)), ('tts_set_equalizer', (0, 0))
    marks_on, marks_off = ('tts_set_token_times', (1, 0, 4)), ('tts_set_token_times', (0, 0, 4))
    for method in sorted(S.CALLS):
        del eng.lib.calls[:]
        S.run(eng, method, equalizer='telephony')
        assert eng.lib.trace() == [on, S.CALLS[method], off] and eng._equalizer is None
        del eng.lib.calls[:]
        S.run(eng, method, equalizer=[('peak', 3000.0, 1.0, 3.0)], limiter=(0.5, 1.0, 1), token_times=True, **S.ALL)
        trace = eng.lib.trace()
        k = trace.index(S.CALLS[method])
        assert trace[k - 1] == ('tts_set_equalizer', (1, 1)) and trace[k + 1] == off                # set last, put back first
        assert trace[k - 2][0] == 'tts_set_token_times' and trace[k + 2][0] == 'tts_set_token_times'
        assert trace[:len(S.ORDER)] == [S.SET[key][0] for key in S.ORDER] and trace[-len(S.ORDER):] == [S.SET[key][1] for key in reversed(S.ORDER)]
        assert eng._equalizer is None
    eng.set_equalizer('warm')
    assert eng._equalizer == ('profile', 'warm') and eng.lib.trace()[-1] == ('tts_set_equalizer', (1, 2))
    del eng.lib.calls[:]
    S.run(eng, 'synthesize', equalizer='warm')                    # equal to the handle's: nothing is set
    assert eng.lib.trace() == [S.CALLS['synthesize']]
    S.run(eng, 'synthesize', equalizer='rumble')
    assert eng.lib.trace()[1:] == [('tts_set_equalizer', (1, 1)), S.CALLS['synthesize'], ('tts_set_equalizer', (1, 2))] and eng._equalizer == ('profile', 'warm')
    eng.set_equalizer(False)
    assert eng._equalizer is None and eng.lib.trace()[-1] == off
    # a setting the library refuses leaves the mirror as it was
    eng.lib.refuse['tts_set_equalizer'] = H.TTS_ERR_INVALID
    with pytest.raises(H.TtsError):
        eng.set_equalizer('bright')
    assert eng._equalizer is None


def test_the_keyword_is_threaded_through_the_helpers_and_the_command_line():
    inf, serve = pkg('tacotron.inference'), pkg('tacotron.serve')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host, inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences, inf.synthesize_text,
               inf.synthesize_texts, inf.synthesize_marked, serve.serve, serve.post_process_spectrograms, inf.SynthSettings):
        assert inspect.signature(fn).parameters['equalizer'].default is None, fn
    assert inf.SETTING_KEYWORDS[-1] == 'equalizer'
    hp = pkg('tacotron.params').model_params
    s = inf.SynthSettings(hp, equalizer='telephony', limiter=0.5)
    assert s.equalizer == ('profile', 'telephony') and s.engine_keywords()['equalizer'] == s.keywords()['equalizer'] == s.host_keywords()['equalizer'] == s.equalizer
    assert inf.SynthSettings(hp).equalizer is None and inf.SynthSettings(hp).equalizer is None
    assert inf.SynthSettings(hp).engine_keywords()['equalizer'] is None
    for bad in ('phone', [('lowpass', 0.6 * hp.sampling_rate)], np.zeros((2, 4))):      # refused before a model is made
        with pytest.raises(ValueError):
            inf.SynthSettings(hp, equalizer=bad)
        with pytest.raises(ValueError):
            inf.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', equalizer=bad)
        with pytest.raises(ValueError):
            next(serve.serve(iter([['x']]), '/nonexistent/weights', equalizer=bad))
    # the command line
    assert inf.parse_args([]).eq is None and inf.settings_option(inf.parse_args([]))['equalizer'] is None
    assert inf.settings_option(inf.parse_args(['--eq', 'telephony']))['equalizer'] == 'telephony'
    eq = inf.settings_option(inf.parse_args(['--eq', 'highpass:120,peak:3000:1.0:+3,highshelf:6000:+2,lowpass:9000:0.5']))['equalizer']
    assert eq == [('highpass', 120.0), ('peak', 3000.0, 1.0, 3.0), ('highshelf', 6000.0, None, 2.0), ('lowpass', 9000.0, 0.5)]
    assert H.equalizer_setting(eq) == ('design', (('highpass', 120.0, H.EQ_Q_BUTTER2, 0.0), ('peak', 3000.0, 1.0, 3.0),
                                                  ('highshelf', 6000.0, H.EQ_Q_BUTTER2, 2.0), ('lowpass', 9000.0, 0.5, 0.0)))
    for bad in ('peak:3000:1:3:9', 'highpass:120:0.7:3', 'peak:', 'peak:abc', 'highpass'):
        with pytest.raises(ValueError):
            H.equalizer_setting(inf.eq_option(bad))


def test_the_finishing_tail_runs_the_equaliser_behind_the_peak_normalisation_and_ahead_of_the_rest():
    """on an engine that records its calls, as tests/test_helpers_host.py holds the tail"""
    import test_helpers_host as T
    inf = pkg('tacotron.inference')
    hp = pkg('tacotron.params').model_params

    class Eng(T.TailEngine):
        def equalize(self, rows, sections, n_samples=None, out=None):
            self.note('equalize', n_samples, sections=np.asarray(sections))
            return rows

    held = np.array([T.HOP * 29, T.HOP * 11], np.int32)
    rows = T.Dev(np.zeros((2, T.HOP * 29), np.float32))
    for settings, peak, want in ((dict(equalizer='telephony'), True, ['peak_normalize', 'equalize']),
                                 (dict(equalizer='telephony'), False, ['equalize']),
                                 (dict(equalizer='warm', loudness=-20.0, limiter=0.5), True, ['equalize', 'loudness_normalize', 'limit']),
                                 (dict(loudness=-20.0), True, ['loudness_normalize']), (dict(), True, ['peak_normalize'])):
        eng = Eng()
        inf.finishing_tail('test', inf.SynthSettings(hp, **settings), T.SR)(eng, rows, held, peak_normalize=peak)
        names = [name for name, _n in eng.calls if name in ('peak_normalize', 'equalize', 'loudness_normalize', 'limit')]
        assert names == want, (settings, names)
        if 'equalize' in want:
            assert dict(eng.calls)['equalize'] == held.tolist()
            assert np.array_equal(eng.kept['equalize']['sections'], pkg('_hip').equalizer_profile(settings['equalizer'], T.SR))
    with pytest.raises(ValueError, match='bright'):
        inf.finishing_tail('test', inf.SynthSettings(None, equalizer='bright'), 8000)
