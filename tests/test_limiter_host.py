"""The limiter and the true-peak meter without a GPU: what the oracle (tests/limiter_oracle.py) promises on the test inputs, how
well the 4x interpolator reads tones, the library's symbols, record and refusals -- made on the arguments alone, with a NULL
handle -- the refusals of every Python layer, and the command line."""
import ctypes
import inspect

import numpy as np
import pytest

import limiter_cases as C
import limiter_oracle as O
from conftest import pkg
from host_checks import no_device_engine


@pytest.fixture(scope='module')
def taps():
    return pkg('_hip').true_peak_filter()


# ---------------------------------------------------------------------------------------------- the oracle's properties
CASES = [(n, L) for L in (0, 1, 7, 110) for n in (O.TILE + 1, 2 * O.TILE + 3)] + [(700, O.MAX_LOOKAHEAD)]


@pytest.mark.parametrize('oversample', [1, 4])
def test_no_finite_sample_ends_above_the_ceiling(taps, oversample):
    cf = O.ceiling_float(C.CEILING)
    assert cf == np.float32(0.5)
    for x, L in [(C.kitchen(n, L), L) for n, L in CASES] + [(C.specials(3000), 7), (C.speech_like(5000, 1.6), 110)]:
        out, (over, limited, min_gain) = O.limit(x, taps, C.CEILING, L, oversample)
        finite = np.isfinite(x)
        assert np.all(np.abs(out[finite]) <= cf) and np.array_equal(C.bits(out[~finite]), C.bits(x[~finite]))
        assert over > 0 and limited >= over and 0.0 < min_gain < 1.0
        # a sample keeps its sign, never grows, and is untouched further than 2 L from anything over the ceiling
        assert np.all(np.signbit(out[finite]) == np.signbit(x[finite])) and np.all(np.abs(out[finite]) <= np.abs(x[finite]))
        a = O.envelope(x, taps, oversample)
        near = np.zeros(len(x), bool)
        for i in np.flatnonzero(a > C.CEILING):
            near[max(0, i - 2 * L):i + 2 * L + 1] = True
        assert np.array_equal(C.bits(out[~near]), C.bits(x[~near]))
    # a ceiling that is no float: the bound is the float under it
    out, _ = O.limit(C.speech_like(3000, 1.6), taps, 0.1, 7, oversample)
    assert O.ceiling_float(0.1) < 0.1 and np.abs(out).max() == O.ceiling_float(0.1)


def test_a_row_under_the_ceiling_comes_back_as_its_bits(taps):
    x = C.quiet(5000)
    x[7] = -0.0
    for oversample in (1, 4):
        for L in (0, 7, 110):
            out, stats = O.limit(x, taps, C.CEILING, L, oversample)
            assert np.array_equal(C.bits(out), C.bits(x)) and stats == (0, 0, 1.0)


def test_phase_0_is_the_impulse_and_the_true_peak_is_never_below_the_sample_peak(taps):
    assert taps.shape == (4, 12) and np.array_equal(taps[0], np.eye(12)[5])
    assert np.all(taps[1:] != 0.0) and np.allclose(taps[1], taps[3][::-1], rtol=0, atol=1e-15) and np.allclose(taps[2], taps[2][::-1], rtol=0, atol=1e-15)
    for x in (C.speech_like(3000, 0.9), C.specials(3000), C.with_peaks(5, [0, 4]), np.zeros(10, np.float32)):
        y = O.interpolate(x, taps)
        assert np.array_equal(y[:, 0], x.astype(np.float64), equal_nan=True)
        tp, sp = O.true_peak(x, taps)
        assert tp >= sp and sp == float(np.max(np.abs(x[np.isfinite(x)]), initial=0.0))
    assert O.true_peak(np.full(4, np.nan, np.float32), taps) == (0.0, 0.0)


def _fir_error(taps, f):
    """the largest error of an interpolated point of a unit tone at f (in units of the sampling rate), whatever its phase:
    max over p of |H_p(f) - exp(2 pi i f p / 4)|, H_p the phase's frequency response about the sample"""
    k = np.arange(O.TAPS) - O.BEFORE
    return max(abs(np.sum(taps[p] * np.exp(2j * np.pi * f * k)) - np.exp(2j * np.pi * f * p / 4.0)) for p in range(1, O.PHASES))


def test_the_true_peak_between_the_samples(taps):
    """sin(pi n / 2 + pi / 4): every sample is +-0.7071, every peak 1.0 lies midway between two"""
    x = np.sin(np.pi * np.arange(400) / 2 + np.pi / 4).astype(np.float32)
    reading = float(np.abs(O.interpolate(x, taps)[50:-50]).max())
    sample_peak = float(np.abs(x).max())
    assert abs(sample_peak - np.sqrt(0.5)) < 1e-7
    e = _fir_error(taps, 0.25)
    assert e < 0.006                                         # (0.0054)
    assert abs(reading - 1.0) <= e + 1e-7, (reading, e)      # the peaks fall on phase 2 exactly; 1e-7: the float32 samples
    assert 20 * np.log10(reading / sample_peak) > 2.9        # the 3 dB a sample-peak meter misses


# What the oracle reads on tones of amplitude 1 at 45 frequencies up to f_max and 33 phases each, 300 interior samples (DESIGN.md
# 4.16): (f_max, the worst under-read 1 - reading of the 12-tap interpolator, that of the exact 4x points -- whose bound is
# 1 - cos(pi f / 4) --, the interpolator's largest error on those tones).  The interpolator's 12 taps leave a transition band
# from about 0.37 to 0.63 of the sampling rate: up to 0.35 it is good to 0.7 %, at 0.45 it has lost a third of the tone and the
# reading falls back on phase 0, the samples themselves.
TONES = [(0.35, 0.0019733, 0.0011327, 0.0069994), (0.45, 0.0489435, 0.0489435, 0.3495746)]


@pytest.mark.parametrize('f_max, under_fir, under_ideal, fir_error', TONES)
def test_the_under_read_on_tones(taps, f_max, under_fir, under_ideal, fir_error):
    got_fir = got_ideal = got_error = 0.0
    for f, _ph, x, exact in C.tones(f_max):
        y, e = O.interpolate(x, taps)[50:-50], exact[50:-50]
        r_fir, r_ideal = float(np.abs(y).max()), float(np.abs(e).max())
        got_fir, got_ideal, got_error = max(got_fir, 1.0 - r_fir), max(got_ideal, 1.0 - r_ideal), max(got_error, float(np.abs(y - e).max()))
        # tone by tone: the exact points never read below the bound, and the interpolator is no further from them than its
        # response says (1e-6: float32 samples)
        assert 1.0 - r_ideal <= 1.0 - np.cos(np.pi * f / 4.0) + 1e-12
        assert abs(r_fir - r_ideal) <= _fir_error(taps, f) + 1e-6, f
        assert r_fir >= float(np.abs(x[50:-50]).max())       # never below the sample peak
    print('f_max %.2f: under-read %.7f (exact 4x points %.7f), interpolator error %.7f' % (f_max, got_fir, got_ideal, got_error))
    # the bars: the recorded readings plus the interpolator's own recorded error doubled
    assert got_ideal <= under_ideal + 2 * fir_error and got_fir <= under_fir + 2 * fir_error
    # ... and the records are what is measured (7 digits were written down)
    assert abs(got_fir - under_fir) < 1e-6 and abs(got_ideal - under_ideal) < 1e-6 and abs(got_error - fir_error) < 1e-6


# ---------------------------------------------------------------------------------------------- the library, without a device
NAMES = ('tts_true_peak', 'tts_true_peak_filter', 'tts_limit', 'tts_limit_max_lookahead', 'tts_set_limiter')


def test_symbols_and_the_record():
    H = pkg('_hip')
    lib = H.load_library()
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert lib.tts_limit_max_lookahead() == O.MAX_LOOKAHEAD == H.LIMIT_MAX_LOOKAHEAD
    assert lib.tts_true_peak_filter(None) == H.TTS_ERR_INVALID
    assert ctypes.sizeof(H.TtsLimitStats) == 16 == H.LIMIT_RECORD.itemsize
    assert [(n, H.LIMIT_RECORD.fields[n][1]) for n in H.LIMIT_RECORD.names] == [('over', 0), ('limited', 4), ('min_gain', 8)]
    assert (H.TtsLimitStats.over.offset, H.TtsLimitStats.limited.offset, H.TtsLimitStats.min_gain.offset) == (0, 4, 8)
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[keys.index('limiter')]
    assert (row.mirror, row.initial, row.host_only) == ('_limiter', None, False) and row.check is H.limiter_setting
    assert keys[keys.index('limiter') - 1:keys.index('limiter') + 2] == ['alignment_stats', 'limiter', 'output']
    assert no_device_engine()._limiter is None


def _i32(values):
    arr = (ctypes.c_int32 * len(values))(*values)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), arr


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal is made on the arguments alone, ahead of the handle: with a NULL handle a bad call and a good one are both
    refused, but only the bad one with its own reason.  The pointers are never dereferenced."""
    H = pkg('_hip')
    lib = H.load_library()
    INV = H.TTS_ERR_INVALID
    p = 4096   # any aligned non-NULL address
    nan, inf = float('nan'), float('inf')

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    good, _k = _i32([5000, 1, 275])
    assert lib.tts_true_peak(None, p, 3, 5000, good, p, p) == INV                  # a good call: only the handle is missing
    for args, text in (
            ((None, 3, 5000, None, p, None), 'true_peak: a NULL pointer (wav and true_peak are required)'),
            ((p, 3, 5000, None, None, p), 'true_peak: a NULL pointer (wav and true_peak are required)'),
            ((p, 0, 5000, None, p, None), 'true_peak: need B, N >= 1'),
            ((p, 3, 0, None, p, None), 'true_peak: need B, N >= 1'),
            ((p, 3, 5000, _i32([5000, 0, 275])[0], p, None), 'true_peak: n_samples[1] = 0 is not in 1 .. N = 5000'),
            ((p, 3, 5000, _i32([5000, 1, 5001])[0], p, None), 'true_peak: n_samples[2] = 5001 is not in 1 .. N = 5000'),
            ((p + 2, 3, 5000, None, p, None), 'true_peak: true_peak and sample_peak must be 8-byte aligned'),
            ((p, 3, 5000, None, p + 4, None), 'true_peak: true_peak and sample_peak must be 8-byte aligned'),
            ((p, 3, 5000, None, p, p + 4), 'true_peak: true_peak and sample_peak must be 8-byte aligned')):
        assert lib.tts_true_peak(None, *args) == INV and why().startswith(text), (args, why())
    assert lib.tts_limit(None, p, 3, 5000, good, 0.5, 110, 4, p) == INV
    for args, text in (
            ((None, 3, 5000, None, 0.5, 110, 4, None), 'limit: a NULL pointer (wav is required)'),
            ((p, 0, 5000, None, 0.5, 110, 4, None), 'limit: need B, N >= 1'),
            ((p, 3, -1, None, 0.5, 110, 4, None), 'limit: need B, N >= 1'),
            ((p, 3, 5000, None, 0.0, 110, 4, None), 'limit: the ceiling must be finite and positive'),
            ((p, 3, 5000, None, -0.5, 110, 4, None), 'limit: the ceiling must be finite and positive'),
            ((p, 3, 5000, None, nan, 110, 4, None), 'limit: the ceiling must be finite and positive'),
            ((p, 3, 5000, None, inf, 110, 4, None), 'limit: the ceiling must be finite and positive'),
            ((p, 3, 5000, None, 0.5, -1, 4, None), 'limit: the look-ahead -1 is not in 0 .. 1024'),
            ((p, 3, 5000, None, 0.5, 1025, 4, None), 'limit: the look-ahead 1025 is not in 0 .. 1024'),
            ((p, 3, 5000, None, 0.5, 110, 2, None), 'limit: oversample must be 1 or 4'),
            ((p, 3, 5000, None, 0.5, 110, 0, None), 'limit: oversample must be 1 or 4'),
            ((p, 3, 5000, _i32([5000, -1, 275])[0], 0.5, 110, 4, None), 'limit: n_samples[1] = -1 is not in 1 .. N = 5000'),
            ((p + 2, 3, 5000, None, 0.5, 110, 4, None), 'limit: stats must be 8-byte aligned, wav 4-byte aligned'),
            ((p, 3, 5000, None, 0.5, 110, 4, p + 4), 'limit: stats must be 8-byte aligned, wav 4-byte aligned')):
        assert lib.tts_limit(None, *args) == INV and why().startswith(text), (args, why())
    assert lib.tts_set_limiter(None, 1, 0.5, 110, 4) == INV and lib.tts_set_limiter(None, 0, 1.0, 0, 1) == INV


# ---------------------------------------------------------------------------------------------- the Python surface
def test_the_python_surface_refuses_before_it_touches_a_handle():
    H = pkg('_hip')
    eng = no_device_engine()
    X = np.zeros((2, 5000), np.float32)
    for call, text in (
            (lambda: eng.true_peak(np.zeros((1, 2, 3), np.float32)), 'true_peak: one waveform (n,) or a batch (B, n) is needed, got shape (1, 2, 3)'),
            (lambda: eng.true_peak(X, n_samples=[5000, 0]), 'n_samples[1] = 0 is not in 1 .. n = 5000'),
            (lambda: eng.true_peak(X, n_samples=[5000]), 'n_samples: 2 integers are needed, got shape (1,) of int64'),
            (lambda: eng.limit(X, 0.0), 'limit: the ceiling must be finite and positive, got 0.0'),
            (lambda: eng.limit(X, float('nan')), 'limit: the ceiling must be finite and positive, got nan'),
            (lambda: eng.limit(X, float('inf')), 'limit: the ceiling must be finite and positive, got inf'),
            (lambda: eng.limit(X, 'loud'), "limit: the ceiling must be a number, got 'loud'"),
            (lambda: eng.limit(X, 0.5, -1), 'limit: the look-ahead must be an integer in 0 .. 1024 samples, got -1'),
            (lambda: eng.limit(X, 0.5, 1025), 'limit: the look-ahead must be an integer in 0 .. 1024 samples, got 1025'),
            (lambda: eng.limit(X, 0.5, 7.5), 'limit: the look-ahead must be an integer in 0 .. 1024 samples, got 7.5'),
            (lambda: eng.limit(X, 0.5, 7, 2), 'limit: oversample must be 1 or 4, got 2'),
            (lambda: eng.limit(X, 0.5, 7, True), 'limit: oversample must be 1 or 4, got True'),
            (lambda: eng.limit(X, 0.5, 7, 4, n_samples=[5000, 5001]), 'n_samples[1] = 5001 is not in 1 .. n = 5000'),
            (lambda: eng.set_limiter(-1.0), 'limiter: the ceiling must be finite and positive, got -1.0'),
            (lambda: eng.set_limiter((0.5, 5.0)), 'limiter must be None, a ceiling or (ceiling, lookahead_ms, oversample), got (0.5, 5.0)'),
            (lambda: eng.set_limiter((0.5, -1.0, 4)), 'limiter: the look-ahead must be finite and not negative, got -1.0'),
            (lambda: eng.set_limiter((0.5, 5.0, 3)), 'limiter: oversample must be 1 or 4, got 3'),
            (lambda: eng.set_limiter(True), 'limiter: the ceiling must be a number, got True'),
            (lambda: eng.set_limiter((0.5, 50.0, 4)), 'set_limiter: a look-ahead of 50.0 ms is 1102 samples at 22050 Hz, more than 1024'),
            (lambda: pkg('audio.effects').limit(X, 0.5, 48000, 25.0, engine=eng), 'limit: a look-ahead of 25.0 ms is 1200 samples at 48000 Hz, more than 1024')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert H.limiter_setting(None) is None and H.limiter_setting(0.5) == (0.5, 5.0, 4) and H.limiter_setting((1, 0, 1)) == (1.0, 0.0, 1)
    assert H.limiter_lookahead('x', 5.0, 22050) == 110 and H.limiter_lookahead('x', 0.0, 22050) == 0 and H.limiter_lookahead('x', 46.4, 22050) == 1023
    assert H.dbtp(0.0) == -np.inf and abs(H.dbtp(0.5) + 6.0206) < 1e-4
    # the synthesis calls check the keyword before anything else is looked at
    ids = np.zeros((1, 4), np.int32)
    for bad in (float('nan'), 0.0, (0.5, 5.0), 'loud', (0.5, 5.0, 2)):
        with pytest.raises(ValueError):
            eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, limiter=bad)
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, limiter=bad)


def test_the_keyword_is_set_last_and_put_back_first():
    """the eighth row of SETTINGS around a call, on a library that records its calls (as tests/test_settings_host.py holds the
    other seven)"""
    import test_settings_host as S
    H = pkg('_hip')
    eng = no_device_engine()
    eng.lib = S.RecordingLibrary()
    eng.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    eng._staging, eng._host_shapes, eng._host_out_shapes = {}, {}, {}
    on, off = ('tts_set_limiter', (1, 0.5, 110, 4)), ('tts_set_limiter', (0, 1.0, 0, 1))
    for method in sorted(S.CALLS):
        del eng.lib.calls[:]
        S.run(eng, method, limiter=0.5)
        assert eng.lib.trace() == [on, S.CALLS[method], off] and eng._limiter is None
        del eng.lib.calls[:]
        S.run(eng, method, limiter=(0.5, 1.0, 1), **S.ALL)
        assert eng.lib.trace() == ([S.SET[k][0] for k in S.ORDER] + [('tts_set_limiter', (1, 0.5, 22, 1)), S.CALLS[method], off] +
                                   [S.SET[k][1] for k in reversed(S.ORDER)])
    eng.set_limiter((0.25, 2.0, 1))
    assert eng._limiter == (0.25, 2.0, 1)
    del eng.lib.calls[:]
    S.run(eng, 'synthesize', limiter=(0.25, 2.0, 1))            # equal to the handle's: nothing is set
    assert eng.lib.trace() == [S.CALLS['synthesize']]
    eng.set_limiter(False)
    assert eng._limiter is None and eng.lib.trace()[-1] == off


def test_the_keyword_is_threaded_through_the_entry_points():
    inf, serve = pkg('tacotron.inference'), pkg('tacotron.serve')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host, inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences,
               serve.serve, serve.post_process_spectrograms, inf.SynthSettings.__init__):
        assert inspect.signature(fn).parameters['limiter'].default is None, fn
    s = inf.SynthSettings(None, limiter=0.5)
    assert s.limiter == (0.5, 5.0, 4) and s.engine_keywords()['limiter'] == (0.5, 5.0, 4) and s.keywords()['limiter'] == (0.5, 5.0, 4)
    assert inf.SynthSettings(None).engine_keywords()['limiter'] is None
    # ... and refused before a model is made
    for bad in (float('nan'), (0.5, 5.0, 2)):
        with pytest.raises(ValueError):
            inf.synthesize_batch(None, None, limiter=bad)
        with pytest.raises(ValueError):
            next(inf.synthesize_stream(None, [], limiter=bad))
        with pytest.raises(ValueError):
            inf.synthesize_sentences(['a'], None, limiter=bad)
        with pytest.raises(ValueError):
            inf.synthesize_text(None, ['a'], None, limiter=bad)
        with pytest.raises(ValueError):
            next(serve.serve(iter([]), None, limiter=bad))
    assert 'Engine.true_peak' in pkg('audio.metrics').true_peak.__doc__ and 'Engine.limit' in pkg('audio.effects').limit.__doc__


def test_the_command_line_parses():
    inf = pkg('tacotron.inference')
    args = inf.parse_args([])
    assert args.limit is None and args.limit_lookahead_ms == 5.0 and args.sample_peak is False and args.max_peak == 1.0
    args = inf.parse_args(['--limit', '-1', '--limit-lookahead-ms', '2.5', '--sample-peak'])
    assert (args.limit, args.limit_lookahead_ms, args.sample_peak, args.max_peak) == (-1.0, 2.5, True, 1.0)
    # with a loudness target the gain gets 12 dB of headroom for the limiter to take back, unless the caller says otherwise
    assert inf.parse_args(['--limit=-1', '--loudness', '-16']).max_peak == 4.0
    assert inf.parse_args(['--limit=-1', '--loudness', '-16', '--max-peak', '2']).max_peak == 2.0
    assert inf.parse_args(['--loudness', '-16']).max_peak == 1.0
    with pytest.raises(SystemExit):
        inf.parse_args(['--limit'])


# ---------------------------------------------------------------------------------------------- the wrappers, on the oracle
class _OracleEngine(object):
    """Engine.true_peak / limit answered by the oracle"""
    sampling_rate = C.SR

    def __init__(self, taps):
        self.taps, self.calls = taps, []

    def true_peak(self, wavs, n_samples=None, want_sample_peak=False):
        rows = np.atleast_2d(np.asarray(wavs, np.float32))
        return np.array([O.true_peak(r, self.taps)[0] for r in rows])

    def limit(self, wavs, ceiling, lookahead=0, oversample=4, n_samples=None):
        self.calls.append((ceiling, lookahead, oversample))
        wavs = np.asarray(wavs, np.float32)
        out = np.stack([O.limit(r, self.taps, ceiling, lookahead, oversample)[0] for r in np.atleast_2d(wavs)]).reshape(wavs.shape)
        return type('Dev', (), {'to_host': lambda self: out, 'free': lambda self: None})(), None


def test_the_audio_wrappers(taps):
    M, Fx = pkg('audio.metrics'), pkg('audio.effects')
    eng = _OracleEngine(taps)
    tone = np.sin(np.pi * np.arange(400) / 2 + np.pi / 4).astype(np.float32)
    one = M.true_peak(tone, engine=eng)
    assert isinstance(one, float) and 0.0 < one < 0.3                    # about 0 dBTP, where the samples say -3
    both = M.true_peak(np.stack([tone, 0.5 * tone]), engine=eng)
    assert both.shape == (2,) and abs((both[0] - both[1]) - 20.0 * np.log10(2.0)) < 1e-6
    assert M.true_peak(np.zeros(10, np.float32), engine=eng) == -np.inf
    x = C.kitchen(3000, 110)
    out = Fx.limit(x, C.CEILING, engine=eng)
    assert eng.calls[-1] == (C.CEILING, 110, 4) and out.shape == x.shape and np.abs(out).max() <= C.CEILING
    Fx.limit(np.stack([x, x]), C.CEILING, sampling_rate=8000, lookahead_ms=2.0, true_peak=False, engine=eng)
    assert eng.calls[-1] == (C.CEILING, 16, 1)
