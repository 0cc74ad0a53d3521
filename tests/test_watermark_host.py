"""CPU: the watermark above and below the kernels, with no GPU.  The arithmetic of tests/watermark_oracle.py (which the GPU tests hold
the kernels to): the chip-sum detector against the definition, the carrier's properties, the envelope's rules, what a mark of a known
strength scores.  The measured numbers: the threshold from wrong keys, and the robustness chain on the oracles of every stage.
Then the Python layers: the checks of ``_hip``, the settings table and the order in which a call sets and puts back, the keyword
through every helper and both command lines, and the finishing tail's order, on a library and an engine that record their calls.

Measured here (printed by the tests; DESIGN.md 4.24 records them): over 200 wrong keys on each of the four signals of
watermark_cases.signals() at D = 64 the largest zeta is 4.39, so the threshold is 1.5 x 4.39 = 6.6; the rightly keyed rows of the
same signals (20 000 samples at the default strength 0.02) reach 1.19 .. 6.72: under a second of speech at the untuned default
strength is NOT enough.  The robustness chain (strength 0.2, 20 000 samples, limiter, 8 kHz, mu-law and back) gives zeta 41.1 on
the oracles, 6.2 times the threshold, against 1.5 for a wrong key."""
import inspect

import numpy as np
import pytest

import watermark_cases as C
import watermark_oracle as O
from conftest import pkg
from host_checks import no_device_engine


# ---------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize('name', sorted(C.SETS))
def test_the_chip_sum_detector_is_the_definition(name):
    """on small rows: every offset's score, the sums at the offset found, the energy and the payload"""
    p = C.params(name)
    y = O.embed(C.voiced(700, seed=5), p)[0]
    for cut, D in ((0, 1), (3, 9), (p.chip, p.chip + 1), (1, 2 * p.chip + 3)):
        a, b = O.detect(y[cut:], p, D), O.detect_brute(y[cut:], p, D)
        assert (a.offset, a.n, a.score, a.energy, a.payload) == (b.offset, b.n, b.score, b.energy, b.payload), (name, cut, D)
        assert np.array_equal(a.T, b.T) and np.array_equal(a.S, b.S), (name, cut, D)
    for x in (np.zeros(0, np.float32), np.zeros(1, np.float32), C.specials(300)):
        a, b = O.detect(x, p, 5), O.detect_brute(x, p, 5)
        assert (a.offset, a.score, a.energy, a.payload) == (b.offset, b.score, b.energy, b.payload) and np.array_equal(a.T, b.T)


def test_the_carrier():
    p = C.params('default')
    s = O.carrier(p, np.arange(200000))
    assert set(s.tolist()) == {-1, 1}
    L = p.chip
    assert np.all(s.reshape(-1, L).sum(axis=1) == 0)                     # the pulse has no DC, chip by chip
    assert np.all(s.reshape(-1, L)[:, :L // 2] == -s.reshape(-1, L)[:, L // 2:])
    c = O.chip_sign(p.key, np.arange(25000))
    assert abs(int(c.sum())) < 4 * 25000 ** 0.5                          # the signs are balanced ...
    assert abs(int((c[1:] * c[:-1]).sum())) < 4 * 25000 ** 0.5           # ... and neighbours do not agree more often than not
    assert np.array_equal(O.chip_sign(p.key, np.arange(100)), O.chip_sign(p.key, np.arange(100)))
    assert not np.array_equal(O.chip_sign(p.key, np.arange(100)), O.chip_sign(p.key + 1, np.arange(100)))
    # the payload flips whole symbols: bit j of the payload, symbol by symbol
    sym = L * p.chips_per_symbol
    zero = O.carrier(p._replace(payload=0), np.arange(40 * sym))
    flips = (s[:40 * sym] * zero).reshape(40, sym)
    assert np.all(flips == flips[:, :1])
    assert [int(f < 0) for f in flips[:, 0]] == [(p.payload >> (u % p.payload_bits)) & 1 for u in range(40)]


def test_the_envelope_keeps_the_mark_out_of_edges_silence_and_onsets():
    x = np.zeros(64 * 10, np.float32)
    x[64 * 4:64 * 8] = C.voiced(64 * 4, amp=0.5, seed=1)
    x[64 * 4 + 5] = np.inf
    x[64 * 5 + 5] = np.nan
    e = O.envelope(x)
    assert not e[:64 * 5].any() and not e[64 * 7:].any() and np.all(e[64 * 5:64 * 7] > 0)   # the onset block and the last one carry no mark
    y, marked = O.embed(x, C.params('default'))
    assert marked[64 * 5:64 * 7].sum() == 127 and not marked[64 * 5 + 5] and marked.sum() == 127
    assert np.array_equal(C.bits(y[~marked]), C.bits(x[~marked]))
    full = C.voiced(640, seed=2)
    assert not O.envelope(full)[:64].any() and not O.envelope(full)[576:].any()               # ... nor the first and the last block of a row
    assert not O.envelope(C.voiced(128, seed=3)).any() and O.envelope(C.voiced(129, seed=3))[64:128].all()
    assert O.embed_stats(x, C.params('default'))[:2] == (640, 127)


def test_the_strength_is_what_the_detector_sees():
    """a mark on silence-free noise-free ground: a constant row marked at G reads chip sums of 64 G L under the envelope of 1 + G"""
    p = C.params('default', strength=0.125)
    x = np.full(19200, np.float32(0.5))                                  # (the payload of 16 symbols of 512 samples wraps twice)
    y, marked = O.embed(x, p)
    assert marked[64:-64].all()
    v = O.v_of(y)
    a = O.chip_sums(v, p.chip, 0)[16:-24]                                # (the blocks beside the unmarked edge blocks lie under their envelope, 1)
    want = round(64 * 0.125 / 1.125) * p.chip                            # every sample is 64 (1 +- G) / (1 + G): the constant cancels in the pulse
    assert np.all(np.abs(a) == want)
    r = O.detect(y, p, 16)
    assert (r.offset, r.payload) == (0, p.payload) and O.zeta(r.score, r.energy, p.payload_bits) > 50


# ---------------------------------------------------------------------------------------------- the measured numbers
def test_the_threshold_is_one_and_a_half_times_what_wrong_keys_reach():
    """at least 200 wrong keys on every signal of watermark_cases at D = 64; the figures are printed, and the module's docstring and
    DESIGN.md 4.24 record them"""
    H = pkg('_hip')
    p = C.params('default')
    worst, right = 0.0, []
    for name, x in sorted(C.signals().items()):
        y = O.embed(x, p)[0]
        r = O.detect(y, p, 64)
        right.append(O.zeta(r.score, r.energy, p.payload_bits))
        zs = []
        for k in range(200):
            w = O.detect(y, p._replace(key=1000 + k), 64)
            zs.append(O.zeta(w.score, w.energy, p.payload_bits))
        print('%-6s wrong keys: largest zeta %.3f, mean %.3f; the right key: %.3f' % (name, max(zs), float(np.mean(zs)), right[-1]))
        worst = max(worst, max(zs))
    print('largest %.3f, times 1.5: %.3f; rightly keyed rows %.3f .. %.3f' % (worst, 1.5 * worst, min(right), max(right)))
    assert abs(H.WM_THRESHOLD - 1.5 * worst) <= 0.05


def test_the_robustness_chain_passes_on_the_oracles_with_twice_the_threshold():
    H = pkg('_hip')
    p = C.chain_params()
    received = C.chain_on_the_oracles(C.chain_signal(), p)
    r = O.detect(received, p, C.CHAIN_OFFSETS)
    z = O.zeta(r.score, r.energy, p.payload_bits)
    w = O.detect(received, p._replace(key=C.CHAIN_WRONG_KEY), C.CHAIN_OFFSETS)
    zw = O.zeta(w.score, w.energy, p.payload_bits)
    print('zeta %.2f = %.2f thresholds at offset %d, payload 0x%04X; a wrong key: %.2f' % (z, z / H.WM_THRESHOLD, r.offset, r.payload, zw))
    assert (r.offset, r.payload) == (C.CHAIN_CUT, p.payload)
    assert z >= 2.0 * H.WM_THRESHOLD and zw < H.WM_THRESHOLD


# ---------------------------------------------------------------------------------------------- the checks of the binding
def test_the_settings_values_and_their_refusals():
    H = pkg('_hip')
    assert H.WM_DEFAULTS == (None, 0, 16, 8, 64, 0.02) == (None, 0) + tuple(O.DEFAULTS[k] for k in ('payload_bits', 'chip', 'chips_per_symbol', 'strength'))
    assert H.watermark_setting(None) is None
    assert H.watermark_setting(7) == H.watermark_setting((7,)) == H.watermark_setting([7, None]) == (7, 0, 16, 8, 64, 0.02)
    assert H.watermark_setting((2 ** 64 - 1, 2 ** 32 - 1)) == (2 ** 64 - 1, 2 ** 32 - 1, 16, 8, 64, 0.02)
    assert H.watermark_setting((7, 3, 32, 16, 65536, 0.25)) == (7, 3, 32, 16, 65536, 0.25)
    assert H.watermark_setting((np.int64(7), np.uint32(3), 1, 2, 1, 0)) == (7, 3, 1, 2, 1, 0.0)
    assert H.watermark_setting(H.watermark_setting((7, 3))) == H.watermark_setting((7, 3))
    for bad in ('key', 0.5, True, (), (True,), (-1,), (2 ** 64,), (7, -1), (7, 2 ** 32), (7, 0, 0), (7, 0, 33), (7, 0, 16, 0), (7, 0, 16, 7),
                (7, 0, 16, 18), (7, 0, 16, 8, 0), (7, 0, 16, 8, 65537), (7, 0, 16, 8, 64, -0.1), (7, 0, 16, 8, 64, 0.26), (7, 0, 16, 8, 64, float('nan')),
                (7, 0, 16, 8, 64, '0.02'), (7, 0, 16.0), (7, 0, 16, 8, 64, 0.02, 1), np.zeros((2, 4))):
        with pytest.raises(ValueError):
            H.watermark_setting(bad)
    assert H.WATERMARK_EMBED_RECORD.itemsize == 16 and H.WATERMARK_EMBED_RECORD.names == ('n', 'marked', 'peak_out', 'spare')
    assert H.WATERMARK_DETECT_RECORD.itemsize == 32 and H.WATERMARK_DETECT_RECORD.names == ('offset', 'n', 'score', 'energy', 'payload', 'spare')
    assert [f for f, _t in H.TtsWatermark._fields_] == list(O.Params._fields) and H.ctypes.sizeof(H.TtsWatermark) == 32
    assert (H.WM_BITS_MAX, H.WM_CHIP_MIN, H.WM_CHIP_MAX, H.WM_SYMBOL_MAX, H.WM_STRENGTH_MAX, H.WM_MAX_OFFSETS) == \
        (O.BITS_MAX, O.CHIP_MIN, O.CHIP_MAX, O.SYMBOL_MAX, O.STRENGTH_MAX, O.MAX_OFFSETS)
    for score, energy, P in ((0, 0, 16), (1474, 430442, 16), (10 ** 9, 10 ** 12, 32)):
        assert H.watermark_zeta(score, energy, P) == O.zeta(score, energy, P)
    assert H.watermark_zeta(np.int64(5), np.int64(0), 16) == 0.0


def test_the_prototypes():
    H = pkg('_hip')
    P = H._PROTOTYPES
    assert {'tts_watermark_embed', 'tts_watermark_detect', 'tts_watermark_max_offsets', 'tts_set_watermark'} <= set(P)
    assert len(P['tts_watermark_embed'][1]) == 8 and len(P['tts_watermark_detect'][1]) == 10
    assert len(P['tts_set_watermark'][1]) == 3 and P['tts_watermark_max_offsets'][1] == []
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in ('tts_watermark_embed', 'tts_watermark_detect', 'tts_watermark_max_offsets', 'tts_set_watermark'):
        assert 'int ' + name + '(' in header, name
    for name in ('tts_watermark_t', 'tts_watermark_embed_stats_t', 'tts_watermark_detect_t'):
        assert '} ' + name + ';' in header, name
    assert '"watermark"' in header                                       # the profile stage's name


def test_the_engine_refuses_before_the_library_is_touched():
    eng = no_device_engine()
    X = np.zeros((2, 5000), np.float32)
    effects, metrics = pkg('audio.effects'), pkg('audio.metrics')
    for call in (lambda: eng.watermark_embed(X, None), lambda: eng.watermark_embed(X, 'key'), lambda: eng.watermark_embed(np.zeros((1, 2, 3), np.float32), 7),
                 lambda: eng.watermark_embed(X, 7, n_samples=[5000, 5001]), lambda: eng.watermark_embed(X, 7, n_samples=[-1, 5]),
                 lambda: eng.watermark_embed(X, 7, out=X), lambda: eng.watermark_embed(X, (7, 0, 16, 7)),
                 lambda: eng.watermark_detect(X, None), lambda: eng.watermark_detect(X, 7, offsets=0), lambda: eng.watermark_detect(X, 7, offsets=4097),
                 lambda: eng.watermark_detect(X, 7, offsets=2.0), lambda: eng.watermark_detect(X, 7, n_samples=[5001, 0]),
                 lambda: eng.set_watermark('key'), lambda: eng.set_watermark((7, 0, 33)),
                 lambda: effects.watermark(X, -1, engine=eng), lambda: effects.watermark(X, 7, strength=0.5, engine=eng),
                 lambda: metrics.detect_watermark(X, 22050, 2 ** 64, engine=eng), lambda: metrics.detect_watermark(X, 22050, 7, chip=3, engine=eng)):
        with pytest.raises(ValueError):
            call()
    ids = np.zeros((1, 4), np.int32)
    for bad in ('key', 0.5, (7, 0, 16, 7), np.zeros((2, 4))):
        with pytest.raises(ValueError):
            eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, watermark=bad)
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, watermark=bad)


# ---------------------------------------------------------------------------------------------- the settings machinery
def test_the_watermark_row_of_the_settings_table():
    H = pkg('_hip')
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[keys.index('watermark')]
    assert (row.mirror, row.initial, row.host_only) == ('_watermark', None, False) and row.check is H.watermark_setting
    assert keys[keys.index('watermark') - 1:] == ['token_times', 'watermark', 'compressor', 'equalizer']
    assert no_device_engine()._watermark is None


def test_the_keyword_is_set_behind_the_timing_marks_and_ahead_of_the_compressor():
    """the ``watermark`` row of SETTINGS around a call, on a library that records its calls (tests/test_settings_host.py)"""
    import test_settings_host as S
    H = pkg('_hip')
    eng = no_device_engine()
    eng.lib = S.RecordingLibrary()
    eng.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    eng._staging, eng._host_shapes, eng._host_out_shapes = {}, {}, {}

    def flags(trace):
        return [(n, a[0]) if n.startswith('tts_set_') else (n, a) for n, a in trace]

    on, off = ('tts_set_watermark', 1), ('tts_set_watermark', 0)
    for method in sorted(S.CALLS):
        del eng.lib.calls[:]
        S.run(eng, method, watermark=7)
        assert flags(eng.lib.trace()) == [on, S.CALLS[method], off] and eng._watermark is None
        del eng.lib.calls[:]
        S.run(eng, method, watermark=(7, 3), compressor=(-20.0, 4.0), equalizer='telephony', limiter=(0.5, 1.0, 1), token_times=True, **S.ALL)
        trace = flags(eng.lib.trace())
        k = trace.index(S.CALLS[method])
        assert [t[0] for t in trace[k - 4:k]] == ['tts_set_token_times', 'tts_set_watermark', 'tts_set_compressor', 'tts_set_equalizer']
        assert [t[0] for t in trace[k + 1:k + 5]] == ['tts_set_equalizer', 'tts_set_compressor', 'tts_set_watermark', 'tts_set_token_times']
        assert trace[k - 3] == on and trace[k + 3] == off
        assert eng._watermark is None and eng._compressor is None
    eng.set_watermark((7, 3))
    assert eng._watermark == (7, 3, 16, 8, 64, 0.02) and flags(eng.lib.trace())[-1] == on
    del eng.lib.calls[:]
    S.run(eng, 'synthesize', watermark=(7, 3))                           # equal to the handle's: nothing is set
    assert eng.lib.trace() == [S.CALLS['synthesize']]
    S.run(eng, 'synthesize', watermark=8)
    assert flags(eng.lib.trace())[1:] == [on, S.CALLS['synthesize'], on] and eng._watermark == (7, 3, 16, 8, 64, 0.02)
    eng.set_watermark(False)
    assert eng._watermark is None and flags(eng.lib.trace())[-1] == off
    eng.lib.refuse['tts_set_watermark'] = H.TTS_ERR_INVALID              # a setting the library refuses leaves the mirror as it was
    with pytest.raises(H.TtsError):
        eng.set_watermark(7)
    assert eng._watermark is None


def test_the_keyword_is_threaded_through_the_helpers_and_the_command_lines():
    inf, serve, detect = pkg('tacotron.inference'), pkg('tacotron.serve'), pkg('tacotron.detect')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host, inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences, inf.synthesize_text,
               inf.synthesize_texts, inf.synthesize_marked, inf.synthesize_marked_sentences, serve.serve, serve.post_process_spectrograms):
        assert inspect.signature(fn).parameters['watermark'].default is None, fn
    assert inf.SETTING_KEYWORDS[-3:] == ('watermark', 'compressor', 'equalizer')
    hp = pkg('tacotron.params').model_params
    s = inf.SynthSettings(hp, watermark=(7, 3), limiter=0.5)
    assert s.watermark == (7, 3, 16, 8, 64, 0.02)
    assert s.engine_keywords()['watermark'] == s.keywords()['watermark'] == s.host_keywords()['watermark'] == s.watermark
    assert inf.SynthSettings(hp).watermark is None and inf.SynthSettings(hp).watermark is None
    for bad in ('key', (7, 0, 16, 7), np.zeros((2, 4))):                 # refused before a model is made
        with pytest.raises(ValueError):
            inf.SynthSettings(hp, watermark=bad)
        with pytest.raises(ValueError):
            inf.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', watermark=bad)
        with pytest.raises(ValueError):
            next(serve.serve(iter([['x']]), '/nonexistent/weights', watermark=bad))
    with pytest.raises(TypeError):
        inf.inference_stream(None, [], watermark=7).__next__()
    # --watermark
    assert inf.parse_args([]).watermark is None and inf.settings_option(inf.parse_args([]))['watermark'] is None
    assert inf.settings_option(inf.parse_args(['--watermark', '0x5EED:0xA5C3']))['watermark'] == (0x5EED, 0xA5C3)
    assert inf.settings_option(inf.parse_args(['--watermark', '12345']))['watermark'] == (12345, 0)
    assert H.watermark_setting(inf.watermark_option('7:3')) == (7, 3, 16, 8, 64, 0.02)
    for bad in ('', 'key', '7:', '7:3:16', '7.5', '-1', '7:-2', '0x10000000000000000'):
        with pytest.raises(ValueError):
            H.watermark_setting(inf.watermark_option(bad))
    # the detector's command line
    args = detect.parse_args(['--key', '0x5EED', 'a.wav', 'b.wav'])
    assert (args.key, args.offsets, args.threshold, args.files) == (0x5EED, 64, H.WM_THRESHOLD, ['a.wav', 'b.wav'])
    assert detect.parse_args(['--key', '7', '--offsets', '4096', '--threshold', '9', 'a.wav']).offsets == 4096
    for bad in (['a.wav'], ['--key', 'k', 'a.wav'], ['--key', '-1', 'a.wav'], ['--key', '7'], ['--key', '7', '--offsets', '0', 'a.wav'],
                ['--key', '7', '--offsets', '4097', 'a.wav']):
        with pytest.raises(SystemExit):
            detect.parse_args(bad)
    assert detect.line('a.wav', dict(detected=True, zeta=12.345, offset=37, payload=0xA5C3)) == 'a.wav\tdetected\tzeta=12.35\toffset=37\tpayload=0xA5C3'
    assert detect.line('b.wav', dict(detected=False, zeta=-0.5, offset=0, payload=3)).split('\t')[1:] == ['absent', 'zeta=-0.50', 'offset=0', 'payload=0x0003']


def test_the_finishing_tail_marks_behind_the_compressor_and_ahead_of_the_loudness():
    """on an engine that records its calls, as tests/test_helpers_host.py holds the tail; that file's TailEngine has no ``watermark_embed``"""
    import test_helpers_host as T
    inf = pkg('tacotron.inference')
    hp = pkg('tacotron.params').model_params
    assert not hasattr(T.TailEngine, 'watermark_embed')

    class Eng(T.TailEngine):
        def equalize(self, rows, sections, n_samples=None, out=None):
            self.note('equalize', n_samples)
            return rows

        def compress(self, rows, params, n_samples=None, out=None, envelope=False):
            self.note('compress', n_samples)
            return rows

        def watermark_embed(self, rows, watermark, n_samples=None, out=None, stats=False):
            self.note('watermark_embed', n_samples, watermark=watermark)
            return rows

    held = np.array([T.HOP * 29, T.HOP * 11], np.int32)
    rows = T.Dev(np.zeros((2, T.HOP * 29), np.float32))
    stages = ('peak_normalize', 'equalize', 'compress', 'watermark_embed', 'loudness_normalize', 'limit')
    for settings, peak, want in ((dict(watermark=7), True, ['peak_normalize', 'watermark_embed']),
                                 (dict(watermark=7), False, ['watermark_embed']),
                                 (dict(watermark=(7, 3), compressor=(-20.0, 4.0), equalizer='warm', loudness=-20.0, limiter=0.5), True,
                                  ['equalize', 'compress', 'watermark_embed', 'loudness_normalize', 'limit']),
                                 (dict(compressor='speech', loudness=-20.0), True, ['compress', 'loudness_normalize'])):
        eng = Eng()
        inf.finishing_tail('test', inf.SynthSettings(hp, **settings), T.SR)(eng, rows, held, peak_normalize=peak)
        names = [name for name, _n in eng.calls if name in stages]
        assert names == want, (settings, names)
        if 'watermark_embed' in want:
            assert dict(eng.calls)['watermark_embed'] == held.tolist()
            assert eng.kept['watermark_embed']['watermark'] == pkg('_hip').watermark_setting(settings['watermark'])
    # with the setting off the tail runs on engines that have no such method
    inf.finishing_tail('test', inf.SynthSettings(hp, loudness=-20.0, limiter=0.5), T.SR)(T.TailEngine(), rows, held, peak_normalize=True)
