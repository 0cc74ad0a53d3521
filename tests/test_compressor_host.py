"""CPU: the compressor above and below the kernels, with no GPU.  The arithmetic of tests/compressor_oracle.py (which the GPU tests
hold the kernels to): the segmented envelope against the plain sequential recurrence, the identities, the static curve on a
two-level tone, the rise and fall times, and the two facts the GPU bound on the output rests on.  Then the Python layers: the
checks of ``_hip``, the five settings tables and the order in which a call sets and puts back, the keyword through every helper and
the command line, and the finishing tail's order, on a library and an engine that record their calls.

The cut's error, measured here at the corners of attack 0 .. 20 ms, release 0 .. 2000 ms and 8 .. 192 kHz: at worst 1.4e-14 of the
row's largest envelope value (attack 20 ms, release 2000 ms, 8 kHz; 4e-15 was an earlier probe's figure), against the cap of 2^-30."""
import inspect
import math

import numpy as np
import pytest

import compressor_cases as C
import compressor_oracle as O
from conftest import pkg
from host_checks import no_device_engine


# ---------------------------------------------------------------------------------------------- the arithmetic
CORNERS = [(a, r, sr) for a in (0.0, 20.0) for r in (0.0, 2000.0) for sr in (8000, 192000)] + [(5.0, 100.0, 22050), (0.5, 2000.0, 48000)]


def test_the_segmented_envelope_stays_within_the_cap_of_the_plain_recurrence():
    """the chains multiply aR and aA out 256 times instead of applying them 256 times: a few roundings per segment, not a drift.
    The figure of every corner is printed; the module's docstring records the worst."""
    worst = 0.0
    x = np.concatenate([C.burst(3000), C.speech_like(2500, amp=1.2), np.zeros(1500, np.float32), C.speech_like(1300, amp=0.2, seed=4)])
    for attack, release, sr in CORNERS:
        p = O.params(-20.0, 4.0, 6.0, attack, release, 0.0, sr)
        w = O.compress(x, p)
        plain = O.plain(x, p)
        err = float(np.abs(w.envelope - plain).max() / plain.max())
        print('attack %g ms, release %g ms, %d Hz: %.3g of max e' % (attack, release, sr, err))
        assert err <= 2.0 ** -30, (attack, release, sr, err)
        worst = max(worst, err)
    print('worst: %.3g' % worst)


def test_an_overtaken_release_stays_overtaken():
    """max(c, AR s) is the release state a segment ends in: against the plain recurrence run from the true state, for carried-in
    states below, between and above the segment's own peaks"""
    p = C.params('slow')
    k = O.coef(p)
    x = C.speech_like(O.SEG, amp=0.5).astype(np.float64)
    c, _e = np.float64(0.0), np.float64(0.0)
    for v in x:
        c, _e = O.detect(k, v, c, _e)
    for s in (0.0, 1e-3, float(c), 0.9, 5.0):
        e1 = np.float64(s)
        for v in x:
            e1, _e = O.detect(k, v, e1, np.float64(0.0))
        got = float(O.chain_release(k, c, np.float64(s)))
        assert abs(got - float(e1)) <= 2.0 ** -40 * got, s


def test_ratio_one_and_rows_under_the_knee_are_identities():
    x = C.specials(1500)
    w = O.compress(x, C.params('unity'))
    assert w.identity.all() and C.same(w.out, x)
    quiet = C.speech_like(3000, amp=0.01)
    for name in ('speech', 'soft', 'hard', 'slow'):
        p = C.params(name)._replace(makeup_db=0.0)
        assert np.abs(quiet).max() < 10.0 ** ((p.threshold_db - p.knee_db / 2.0) / 20.0)
        w = O.compress(quiet, p)
        assert w.identity.all() and np.array_equal(C.bits(w.out), C.bits(quiet)) and not np.any(w.r < 0), name
    silence = np.zeros(700, np.float32)
    silence[5] = -0.0
    w = O.compress(silence, C.params('speech'))             # e = 0: L = -inf, r = 0 and not NaN; 0 * g keeps its sign
    assert not np.any(np.isnan(w.y)) and np.array_equal(C.bits(w.out), C.bits(silence)) and np.all(w.r == 0)


@pytest.mark.parametrize('name', ['speech', 'soft', 'hard', 'instant_attack'])
def test_the_steady_state_gain_on_a_two_level_tone_is_the_static_curve(name):
    """a tone of 20 samples a cycle, whose peaks are samples: -40 dB (under every knee: the make-up alone), then -6 dB, then -40 dB
    again.  Between two peaks, 10 samples apart, the release lets the envelope droop by aR^10, so the level lies in
    [peak - droop, peak] and the gain within (1 - slope) * droop of the static curve there."""
    sr = 22050
    p = C.params(name)
    x, up, down = C.two_level(sr, -40.0, -6.0, f=sr / 20.0)
    w = O.compress(x, p)
    droop = -20.0 * math.log10(p.release_coeff ** 10) if p.release_coeff > 0 else 400.0
    peaks = np.nonzero(np.arange(len(x)) % 10 == 5)[0]
    with np.errstate(all='ignore'):
        gain_db = 20.0 * np.log10(w.y[peaks] / x[peaks].astype(np.float64))
    loud = gain_db[(peaks > down - 2000) & (peaks < down)]
    want = O.static_gain_db(p, -6.0)
    if p.release_coeff > 0:
        assert np.all(loud >= want - 1e-6) and np.all(loud <= want + (1.0 - p.slope) * droop + 1e-6), (name, loud.min(), loud.max(), want)
    else:                                                   # no release: the envelope is |x| itself, exact at the peaks
        assert np.allclose(loud, want, rtol=0, atol=1e-6)
    assert want < p.makeup_db - 3.0
    quiet = gain_db[(peaks > len(x) - 2000)]
    assert np.allclose(quiet, p.makeup_db, rtol=0, atol=1e-9), name
    assert np.allclose(gain_db[(peaks > up - 2000) & (peaks < up)], p.makeup_db, rtol=0, atol=1e-9)


@pytest.mark.parametrize('attack_ms,release_ms,sr', [(5.0, 500.0, 22050), (1.0, 100.0, 48000), (20.0, 2000.0, 8000)])
def test_the_rise_and_fall_times_are_the_attack_and_the_release_asked_for(attack_ms, release_ms, sr):
    """a step from 0 to 0.5 and back: the envelope rises as 1 - aA^n, 10 % to 90 % in ln 9 attack times, and falls as aR^n seen
    through the attack's pole, which lags a slow exponential by about one attack time at both crossings alike -- so the fall, 90 % to
    10 %, is ln 9 release times to within one attack time.  Crossings are read to the sample: two more samples of slack."""
    n_up = int(sr * attack_ms * 1e-3 * 12)
    n_down = int(sr * release_ms * 1e-3 * 4)
    x = np.concatenate([np.zeros(10), np.full(n_up, 0.5), np.zeros(n_down)]).astype(np.float32)
    env = O.compress(x, O.params(-20.0, 4.0, 6.0, attack_ms, release_ms, 0.0, sr)).envelope
    assert abs(env[10 + n_up - 1] - 0.5) < 1e-4
    rise = (np.argmax(env >= 0.45) - np.argmax(env >= 0.05)) / float(sr)
    assert abs(rise - math.log(9.0) * attack_ms * 1e-3) <= 2.0 / sr, rise
    tail = env[10 + n_up:]
    fall = (np.argmax(tail <= 0.05) - np.argmax(tail <= 0.45)) / float(sr)
    assert abs(fall - math.log(9.0) * release_ms * 1e-3) <= attack_ms * 1e-3 + 2.0 / sr, fall


def test_what_the_bound_on_the_output_rests_on():
    """2^-24 |y| + 2^-40 |y| + 2^-150: a log10 that differs by 4 units in the last place moves the oracle by under a quarter of the
    second term, at speech levels and at the largest |L|; the same gain arithmetic in float32 (the logarithm included) breaks the bound
    on most of the elements whose gain depends on the level, which are most elements of every row here.
    Why the rows are what they are: a float32 L is off by up to 2^-24 |L| dB, which moves the gain by (1 - slope) ln 10 / 20 times
    that, relatively -- beyond the 2^-24 the bound allows once (1 - slope) |L| passes some 17 dB on average.  So the rows sit where
    speech does, 30 .. 50 dB under full scale, under thresholds and ratios that keep (1 - slope) |L| at 25 dB and more; at the
    largest |L| it holds whatever the ratio.  (A row near full scale, where L is a few dB, is not told apart this way.)"""
    quiet = C.speech_like(5000, amp=0.1)
    rows = [(quiet, O.params(-50.0, float('inf'), 0.0, 0.0, 0.0, 0.0, 22050)), (quiet, O.params(-60.0, 8.0, 12.0, 1.0, 50.0, 6.0, 22050)),
            ((C.speech_like(3000, amp=1.0).astype(np.float64) * 1e36).astype(np.float32), O.params(-80.0, float('inf'), 0.0, 1.0, 50.0, -24.0, 22050)),
            (C.speech_like(3000, amp=0.01), O.params(-80.0, 8.0, 40.0, 1.0, 50.0, 24.0, 22050))]
    for x, p in rows:
        w = O.compress(x, p)
        moving = ~C.exact_positions(w)
        assert moving.sum() > len(x) // 2
        for ulps in (4, -4):
            moved = O.compress(x, p, ulps=ulps)
            assert np.array_equal(moved.identity, w.identity)
            rel = np.abs(moved.y[moving] - w.y[moving]) / np.abs(w.y[moving])
            assert rel.max() <= 0.25 * 2.0 ** -40, (tuple(p), ulps, rel.max())
        single = O.compress(x, p, gain_dtype=np.float32)
        with np.errstate(all='ignore'):
            broken = np.abs(single.out[moving].astype(np.float64) - w.y[moving]) > C.bound(w.y[moving])
        reduced = w.r[moving] < 0                          # (where the gain depends on the level; elsewhere it is one constant)
        print('float32 breaks the bound on %.3f of the elements being reduced, %.3f of all' % (broken[reduced].mean(), broken.mean()))
        assert reduced.mean() > 0.5 and broken[reduced].mean() > 0.5, (tuple(p), broken[reduced].mean())
        # ... while the oracle's own float32 output is of course inside it
        ok, worst = C.held(w.out, w)
        assert ok and worst <= 1.0


def test_the_gpu_cases_stay_clear_of_the_knees_lower_edge():
    """where the records are held exactly (tests/test_gpu_compressor.py's ragged batch): no level within 1e-9 dB of T - W / 2"""
    p = C.params('speech')
    for n in (1, O.TILE + 300, 255, O.TILE, 513):
        assert C.clear_of_the_knee(O.compress(C.speech_like(n, amp=1.2), p), p), n
    x = C.two_level(22050, -40.0, -21.0)[0]                # (and the check does see a row that is not: a level ON the edge)
    edge = O.compress(np.full(10, np.float32(10.0 ** (-21.0 / 20.0))), O.params(-18.0, 3.0, 6.0, 0.0, 0.0, 0.0, 22050))
    assert len(x) and not C.clear_of_the_knee(edge, p, margin=1e-6)


def test_the_stats_of_a_row():
    p = C.params('hard')
    x = np.array([0.0, 0.05, -0.5, np.nan, 0.2, -0.01], np.float32)
    n, reduced, max_red, peak = O.stats(O.compress(x, p))
    assert (n, reduced) == (6, 2) and abs(max_red - (20.0 * math.log10(0.5) + 20.0)) < 1e-12
    assert abs(float(peak) - 0.1) < 1e-7                   # ratio infinity: what is over the threshold comes out at it


# ---------------------------------------------------------------------------------------------- the checks of the binding
def test_the_settings_values_and_their_refusals():
    H = pkg('_hip')
    assert list(H.CMP_PROFILES) == ['speech', 'telephony', 'small-speaker'] and dict(H.CMP_PROFILES) == O.PROFILES
    assert H.compressor_setting(None) is None and H.compressor_setting('speech') == ('profile', 'speech')
    assert H.compressor_setting((-20, 4)) == ('design', (-20.0, 4.0, 6.0, 5.0, 100.0, 0.0))
    assert H.compressor_setting([-20.0, float('inf'), 0.0, 0.0, 0.0, 3.0]) == ('design', (-20.0, float('inf'), 0.0, 0.0, 0.0, 3.0))
    assert H.compressor_setting(('design', (-20.0, 4.0, 6.0, 5.0, 100.0, 0.0))) == ('design', (-20.0, 4.0, 6.0, 5.0, 100.0, 0.0))
    assert H.compressor_setting(('profile', 'telephony')) == ('profile', 'telephony')
    for name in O.PROFILES:
        for sr in (8000, 22050, 192000):
            assert tuple(H.compressor_params(('profile', name), sr)) == tuple(O.profile(name, sr))
    assert H.compressor_params(H.compressor_setting((-20.0, float('inf'), 0.0, 0.0, 0.0)), 22050) == (-20.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert H.compressor_design(22050, 5.0, 0.0) == (math.exp(-1.0 / (5.0 * 1e-3 * 22050)), 0.0)
    raw = ('params', (-20.0, 0.25, 6.0, 3.0, 0.875, 0.9375))
    assert H.compressor_setting(raw) == raw and H.compressor_params(raw, 22050) == raw[1]
    for bad in ('loud', 0.5, (-20.0,), (-20.0, 0.5), (0.5, 4.0), (-81.0, 4.0), (-20.0, 4.0, 41.0), (-20.0, 4.0, 6.0, -1.0),
                (-20.0, 4.0, 6.0, 5.0, 10001.0), (-20.0, 4.0, 6.0, 5.0, 100.0, 25.0), (-20.0, float('nan')), (-20.0, '4'), (-20.0, True),
                (1, 2, 3, 4, 5, 6, 7), ('params', (-20.0, 0.25, 6.0, 3.0, 1.0, 0.5)), ('params', (-20.0, 1.5, 6.0, 3.0, 0.5, 0.5))):
        with pytest.raises(ValueError):
            H.compressor_setting(bad)
    for bad in (7999, 192001, 22050.0, True):
        with pytest.raises(ValueError):
            H.compressor_design(bad, 5.0, 100.0)
    assert H.COMPRESS_RECORD.itemsize == 16 and H.COMPRESS_RECORD.names == ('n', 'reduced', 'max_reduction_db', 'peak_out')
    assert [f for f, _t in H.TtsCompressor._fields_] == list(O.Params._fields) and pkg('_hip').ctypes.sizeof(H.TtsCompressor) == 48
    assert {'tts_compress', 'tts_compressor_design', 'tts_compressor_profile', 'tts_set_compressor'} <= set(H._PROTOTYPES)


def test_the_engine_refuses_before_the_library_is_touched():
    eng = no_device_engine()
    X = np.zeros((2, 5000), np.float32)
    for call in (lambda: eng.compress(X, None), lambda: eng.compress(X, 'loud'), lambda: eng.compress(np.zeros((1, 2, 3), np.float32), 'speech'),
                 lambda: eng.compress(X, 'speech', n_samples=[5000, 5001]), lambda: eng.compress(X, 'speech', out=X),
                 lambda: eng.compress(X, (-20.0, 0.5)), lambda: eng.set_compressor('loud'), lambda: eng.set_compressor((-20.0, 0.5)),
                 lambda: pkg('audio.effects').compress(X, 7000, 'speech', engine=eng), lambda: pkg('audio.effects').compress(X, 22050, None, engine=eng)):
        with pytest.raises(ValueError):
            call()
    ids = np.zeros((1, 4), np.int32)
    for bad in ('loud', 0.5, (-20.0, 0.5), np.zeros((2, 4))):
        with pytest.raises(ValueError):
            eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, compressor=bad)
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, compressor=bad)


# ---------------------------------------------------------------------------------------------- the settings machinery
def test_the_compressor_row_of_the_settings_table():
    H = pkg('_hip')
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[keys.index('compressor')]
    assert (row.mirror, row.initial, row.host_only) == ('_compressor', None, False) and row.check is H.compressor_setting
    assert keys[keys.index('compressor') - 1:] == ['watermark', 'compressor', 'equalizer']
    assert no_device_engine()._compressor is None


def test_the_keyword_is_set_ahead_of_the_equaliser_and_put_back_behind_it():
    """the ``compressor`` row of SETTINGS around a call, on a library that records its calls (tests/test_settings_host.py): behind the
    timing marks, ahead of the equaliser, which stays the last one set and the first one put back"""
    import test_settings_host as S
    H = pkg('_hip')
    eng = no_device_engine()
    eng.lib = S.RecordingLibrary()
    eng.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    eng._staging, eng._host_shapes, eng._host_out_shapes = {}, {}, {}

    def flags(trace):
        """(name, enabled) of the setters, the call itself as it is"""
        return [(n, a[0]) if n.startswith('tts_set_') else (n, a) for n, a in trace]

    on, off = ('tts_set_compressor', 1), ('tts_set_compressor', 0)
    for method in sorted(S.CALLS):
        del eng.lib.calls[:]
        S.run(eng, method, compressor='speech')
        assert flags(eng.lib.trace()) == [on, S.CALLS[method], off] and eng._compressor is None
        del eng.lib.calls[:]
        S.run(eng, method, compressor=(-20.0, 4.0), equalizer='telephony', limiter=(0.5, 1.0, 1), token_times=True, **S.ALL)
        trace = flags(eng.lib.trace())
        k = trace.index(S.CALLS[method])
        assert trace[k - 1] == ('tts_set_equalizer', 1) and trace[k + 1] == ('tts_set_equalizer', 0)       # the equaliser: last set, first put back
        assert trace[k - 2] == on and trace[k + 2] == off
        assert trace[k - 3][0] == 'tts_set_token_times' and trace[k + 3][0] == 'tts_set_token_times'
        plain = eng.lib.trace()
        assert plain[:len(S.ORDER)] == [S.SET[key][0] for key in S.ORDER] and plain[-len(S.ORDER):] == [S.SET[key][1] for key in reversed(S.ORDER)]
        assert eng._compressor is None and eng._equalizer is None
    eng.set_compressor('telephony')
    assert eng._compressor == ('profile', 'telephony') and flags(eng.lib.trace())[-1] == on
    del eng.lib.calls[:]
    S.run(eng, 'synthesize', compressor='telephony')              # equal to the handle's: nothing is set
    assert eng.lib.trace() == [S.CALLS['synthesize']]
    S.run(eng, 'synthesize', compressor='speech')
    assert flags(eng.lib.trace())[1:] == [on, S.CALLS['synthesize'], on] and eng._compressor == ('profile', 'telephony')
    eng.set_compressor(False)
    assert eng._compressor is None and flags(eng.lib.trace())[-1] == off
    # a setting the library refuses leaves the mirror as it was
    eng.lib.refuse['tts_set_compressor'] = H.TTS_ERR_INVALID
    with pytest.raises(H.TtsError):
        eng.set_compressor('speech')
    assert eng._compressor is None


def test_the_keyword_is_threaded_through_the_helpers_and_the_command_line():
    inf, serve = pkg('tacotron.inference'), pkg('tacotron.serve')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host, inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences, inf.synthesize_text,
               inf.synthesize_texts, inf.synthesize_marked, inf.synthesize_marked_sentences, serve.serve, serve.post_process_spectrograms):
        assert inspect.signature(fn).parameters['compressor'].default is None, fn
    assert inf.SETTING_KEYWORDS[-2:] == ('compressor', 'equalizer')
    hp = pkg('tacotron.params').model_params
    s = inf.SynthSettings(hp, compressor='speech', limiter=0.5)
    assert s.compressor == ('profile', 'speech')
    assert s.engine_keywords()['compressor'] == s.keywords()['compressor'] == s.host_keywords()['compressor'] == s.compressor
    assert inf.SynthSettings(hp).compressor is None and inf.SynthSettings(hp).compressor is None
    assert inf.SynthSettings(hp).engine_keywords()['compressor'] is None
    for bad in ('loud', (-20.0, 0.5), np.zeros((2, 4))):          # refused before a model is made
        with pytest.raises(ValueError):
            inf.SynthSettings(hp, compressor=bad)
        with pytest.raises(ValueError):
            inf.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', compressor=bad)
        with pytest.raises(ValueError):
            next(serve.serve(iter([['x']]), '/nonexistent/weights', compressor=bad))
    with pytest.raises(TypeError):
        inf.inference_stream(None, [], compressor='speech').__next__()     # (the helper that takes two settings alone refuses it)
    # the command line
    assert inf.parse_args([]).compress is None and inf.settings_option(inf.parse_args([]))['compressor'] is None
    assert inf.settings_option(inf.parse_args(['--compress', 'telephony']))['compressor'] == 'telephony'
    got = inf.settings_option(inf.parse_args(['--compress=-18:3:6:5:100:3']))['compressor']
    assert got == (-18.0, 3.0, 6.0, 5.0, 100.0, 3.0) and H.compressor_setting(got) == ('design', got)
    assert H.compressor_setting(inf.compress_option('-20:inf')) == ('design', (-20.0, float('inf'), 6.0, 5.0, 100.0, 0.0))
    for bad in ('-18:', '-18:abc', '1:2:3:4:5:6:7', '-18:0.5', 'speech:3'):
        with pytest.raises(ValueError):
            H.compressor_setting(inf.compress_option(bad))


def test_the_finishing_tail_runs_the_compressor_behind_the_equaliser_and_never_touches_it_without_a_setting():
    """on an engine that records its calls, as tests/test_helpers_host.py holds the tail; that file's TailEngine has no ``compress``"""
    import test_helpers_host as T
    inf = pkg('tacotron.inference')
    hp = pkg('tacotron.params').model_params
    assert not hasattr(T.TailEngine, 'compress')

    class Eq(T.TailEngine):
        def equalize(self, rows, sections, n_samples=None, out=None):
            self.note('equalize', n_samples)
            return rows

    class Eng(Eq):
        def compress(self, rows, params, n_samples=None, out=None, envelope=False):
            self.note('compress', n_samples, params=params)
            return rows

    held = np.array([T.HOP * 29, T.HOP * 11], np.int32)
    rows = T.Dev(np.zeros((2, T.HOP * 29), np.float32))
    stages = ('peak_normalize', 'equalize', 'compress', 'loudness_normalize', 'limit')
    for settings, peak, want in ((dict(compressor='speech'), True, ['peak_normalize', 'compress']),
                                 (dict(compressor='speech'), False, ['compress']),
                                 (dict(compressor=(-20.0, 4.0), equalizer='warm', loudness=-20.0, limiter=0.5), True,
                                  ['equalize', 'compress', 'loudness_normalize', 'limit']),
                                 (dict(equalizer='warm', loudness=-20.0), True, ['equalize', 'loudness_normalize'])):
        eng = Eng()
        inf.finishing_tail('test', inf.SynthSettings(hp, **settings), T.SR)(eng, rows, held, peak_normalize=peak)
        names = [name for name, _n in eng.calls if name in stages]
        assert names == want, (settings, names)
        if 'compress' in want:
            assert dict(eng.calls)['compress'] == held.tolist()
            how, values = eng.kept['compress']['params']
            assert how == 'params' and values == pkg('_hip').compressor_params(pkg('_hip').compressor_setting(settings['compressor']), T.SR)
    # with the setting off the tail runs on engines that have no such method
    for eng, settings in ((T.TailEngine(), dict(loudness=-20.0, limiter=0.5)), (Eq(), dict(equalizer='warm'))):
        inf.finishing_tail('test', inf.SynthSettings(hp, **settings), T.SR)(eng, rows, held, peak_normalize=True)
    with pytest.raises(ValueError):
        inf.finishing_tail('test', inf.SynthSettings(None, compressor='speech'), 7000)
