"""Prosody markup without a GPU: the symbols of the warp and its refusals made before a device is touched; the oracle's own
arithmetic; ``tacotron.prosody`` -- ``parse_markup`` on a fixed table, ``token_attributes`` through the front end's abbreviations,
``segments_of_row`` on hand-made ``start`` arrays, ``warp_position`` at the borders -- and the timing marks of a slowed word and of
a break; the command line of ``tacotron.inference --markup``."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

import warp_cases as C
import warp_oracle as O
from conftest import ROOT, pkg
from host_checks import no_device_engine

NAMES = ('tts_warp_magnitudes', 'tts_warp_plan', 'tts_warp_max_segments', 'tts_warp_tile')
HOP, SR, R = 275, 22050, 5


def _dataset():
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)


# ---------------------------------------------------------------------------------------------- the library and the binding
def test_symbols():
    H = pkg('_hip')
    lib = H.load_library()
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert 'typedef struct tts_warp_segment' in header and '"warp"' in header
    assert lib.tts_warp_max_segments() == H.WARP_MAX_SEGMENTS == O.MAX_SEGMENTS == 4096
    assert lib.tts_warp_tile() == O.TILE == 64 and H.WARP_SEGMENTS_PER_LAUNCH == O.SEGMENTS_PER_LAUNCH
    assert ctypes.sizeof(H.TtsWarpSegment) == H.WARP_SEGMENT.itemsize == 24
    assert [f[0] for f in H.TtsWarpSegment._fields_] == list(H.WARP_SEGMENT.names) == ['row', 'first', 'frames', 'pause', 'step', 'gain']
    for name in ('warp_magnitudes', 'warp_plan', 'warp_max_segments', 'warp_tile'):
        assert callable(getattr(H.Engine, name))
    with open(os.path.join(ROOT, pkg().__name__, 'build.py')) as f:
        build = f.read()
    assert "'warp.hip'" in build and "'warp_plan.h'" in build and "'warp.hip': ['-ffp-contract=off']" in build


def _bad_lists():
    case = C.mixed()
    seg, nf = case['segments'], case['n_frames']
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(seg)]
    return seg, nf, [(edit(0, 0, 1), nf), (edit(5, 0, 1), nf), ([q for q in seg if q[0] != 1], nf), (seg[:-1], nf), (seg, [40, 41, 1]),
                     (edit(9, 2, 19), nf), (edit(1, 1, -1), nf), (edit(2, 2, -3), nf), (edit(2, 3, 4), nf), (edit(0, 3, 0), nf), (edit(2, 4, 16383), nf),
                     (edit(2, 4, 262145), nf), (edit(2, 5, float('nan')), nf), (edit(2, 5, 16.5), nf), ([(0, 0, 1, 0, 65536, 1.0)] * 4097, [40, 23, 1]),
                     (seg[:2], nf)]


def test_the_plan_and_every_refusal_are_the_oracles():
    """the library's tts_warp_plan, the binding's warp_list and the oracle say the same of every list, in the same words"""
    H = pkg('_hip')
    lib = H.load_library()
    seg, nf, bad = _bad_lists()

    def plan(s, n, B=3, T=40):
        q = C.segment_array(H, s)
        n32 = np.asarray(n, np.int32)
        out = np.zeros(B, np.int64)
        rc = lib.tts_warp_plan(q.ctypes.data, len(q), B, T, n32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return rc, out.tolist(), (lib.tts_last_error(None) or b'').decode()

    why, n_out, counts = O.plan(seg, 3, 40, nf)
    assert why is None and plan(seg, nf)[:2] == (H.TTS_OK, n_out)
    q, _nf, got_n, got_c = H.warp_list(seg, 3, 40, nf)
    assert got_n.tolist() == n_out and got_c.tolist() == counts and q.dtype == H.WARP_SEGMENT
    assert H.warp_list(q, 3, 40, nf)[2].tolist() == n_out                                    # (a WARP_SEGMENT array is taken as it is)
    assert [H.warp_count(f, s) for f, s in ((1, 65535), (1, 65536), (1, 65537), (40, 16384), (40, 262144))] == [2, 1, 1, 160, 10]
    assert [H.warp_launches(S) for S in (1, 64, 65, 4096)] == [O.launches(S) for S in (1, 64, 65, 4096)] == [1, 1, 2, 64]
    for s, n in bad:
        why = O.plan(s, 3, 40, n)[0]
        assert why is not None
        rc, _n, text = plan(s, n)
        assert rc == H.TTS_ERR_INVALID and text == 'warp_plan: ' + why, (why, text)
        with pytest.raises(ValueError) as e:
            H.warp_list(s, 3, 40, n)
        assert str(e.value) == (why if why.startswith('n_frames[') else 'warp: ' + why)      # (a length's refusal is the one every stage gives)
    assert len({O.plan(s, 3, 40, n)[0] for s, n in bad}) >= 13
    # with a NULL handle a good call and a bad one are both refused, but only the bad one with its own reason
    p = 4096   # any aligned non-NULL address: never dereferenced
    q = C.segment_array(H, seg)
    n32 = np.asarray(nf, np.int32)
    pn = n32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    lib.tts_create(None, 0, None)
    assert lib.tts_warp_magnitudes(None, p, 3, 3, 40, pn, q.ctypes.data, len(q), 140, p) == H.TTS_ERR_INVALID
    assert not (lib.tts_last_error(None) or b'').decode().startswith('warp')
    for args, text in (((None, 3, 3, 40, pn, q.ctypes.data, len(q), 140, p), 'a NULL pointer (mag, segments and out are required)'),
                       ((p, 3, 0, 40, pn, q.ctypes.data, len(q), 140, p), 'need B, F, T, S >= 1'),
                       ((p, 3, 3, 40, pn, q.ctypes.data, 0, 140, p), 'need B, F, T, S >= 1'),
                       ((p, 3, 3, 40, pn, q.ctypes.data, len(q), 139, p), 'T_out = 139 is below n_out[0] = 140'),
                       ((p, 3, 3, 40, pn, q.ctypes.data, len(q), (1 << 30) + 1, p), 'T_out = 1073741825 is above 2^30 = 1073741824'),
                       ((p + 2, 3, 3, 40, pn, q.ctypes.data, len(q), 140, p), 'the buffers must be 4-byte aligned')):
        assert lib.tts_warp_magnitudes(None, *args) == H.TTS_ERR_INVALID
        assert (lib.tts_last_error(None) or b'').decode() == 'warp_magnitudes: ' + text
    assert O.room(n_out, 139) == 'T_out = 139 is below n_out[0] = 140'


def test_the_python_surface_refuses_before_it_touches_a_handle():
    eng = no_device_engine()
    seg, nf, bad = _bad_lists()
    X = np.zeros((3, 3, 40), np.float32)
    for s, n in bad:
        with pytest.raises(ValueError):
            eng.warp_magnitudes(X, s, n)
        with pytest.raises(ValueError):
            eng.warp_plan(X.shape, s, n)
    for call, text in ((lambda: eng.warp_magnitudes(X[0], seg, nf), 'warp_magnitudes: a non-empty 3-D array is needed, got shape (3, 40)'),
                       (lambda: eng.warp_plan((3, 40), seg, nf), 'warp_plan: the shape of a batch (B, F, T) is needed, got (3, 40)'),
                       (lambda: eng.warp_magnitudes(X, seg, nf, T_out=139), 'warp_magnitudes: T_out = 139 is not in n_out.max() = 140 .. 2^30'),
                       (lambda: eng.warp_magnitudes(X, [(0, 0, 1, 0, 65536)], nf), 'warp: segments must be a WARP_SEGMENT array or rows (row, first, frames, pause, step, gain)'),
                       (lambda: eng.warp_magnitudes(X, [(0, 0, 1.5, 0, 65536, 1.0)], nf),
                        'warp: segment 0 must hold 32-bit integers row, first, frames, pause and step, got (0, 0, 1.5, 0, 65536, 1.0)'),
                       (lambda: eng.warp_magnitudes(X, seg, [40, 23]), 'n_frames: shape (2,) for a batch of 3')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_the_oracles_arithmetic():
    x = np.array([[[1.0, 2.0, 4.0, 8.0]]], np.float32)
    out, n_out = O.warp(x, [(0, 0, 4, 0, 32768, 1.0), (0, 0, 0, 2, 0, 0.0), (0, 1, 2, 0, 131072, 0.5)], None, 12)
    assert n_out == [11] and out[0, 0].tolist() == [1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 4.0, 0.0, 0.0, 1.0, 0.0]      # (8 blends with the 0.0 behind the row)
    # 0 * NaN stays NaN under a == 0, -0.0 + -0.0 is -0.0, a zero gain keeps the sign
    y = np.array([[[-0.0, -0.0, np.nan, 1.0]]], np.float32)
    out, _n = O.warp(y, [(0, 0, 2, 0, 65536, 1.0), (0, 3, 1, 0, 65536, 0.0), (0, 0, 1, 0, 65536, 0.0)], None, 4)
    assert np.isnan(out[0, 0, 1]) and out.view(np.uint32)[0, 0, [0, 2, 3]].tolist() == [0x80000000, 0, 0x80000000]
    # the uniform stretch is contained: lengths and bits
    import stretch_oracle as S
    xx = C.batch(1, 3, 40)[0]
    for q in C.CONTAINED_STEPS:
        for n in range(1, 41):
            assert O.count(n, q) == S.stretched_frames(n, q / 65536.0)
        for n in (1, 7, 40):
            a, b = O.blend_segment(xx, n, 0, O.count(n, q), q, 1.0), S.blend(xx[:, :n], q / 65536.0)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- parse_markup
def test_parse_markup_on_a_fixed_table():
    P = pkg('tacotron.prosody')
    inf = pkg('tacotron.inference')
    assert P.parse_markup('No markup at all.') == ('No markup at all.', [], [])
    plain, spans, breaks = P.parse_markup('Hello <prosody rate="50%">slow <emphasis level="strong">word</emphasis></prosody> and<break time="300ms"/> more &amp; so')
    assert plain == 'Hello slow word and more & so' and breaks == [(19, 300.0)]
    assert spans == [(6, 15, 0.5, 0.0), (11, 15, 0.5 * P.EMPHASIS['strong'][0], P.EMPHASIS['strong'][1])]             # nested rates multiply
    plain, spans, _b = P.parse_markup('a <prosody volume="-6 dB" rate="1.5">b <prosody volume="+2.5dB" rate="fast">c</prosody> <prosody volume="silent">d</prosody></prosody>')
    assert plain == 'a b c d' and spans == [(2, 7, 1.5, -6.0), (4, 5, 1.5 * 1.25, -3.5), (6, 7, 1.5, -math.inf)]       # nested volumes add in dB
    for name, rate in P.RATES.items():
        assert P.parse_markup('<prosody rate="{}">x</prosody>'.format(name))[1] == [(0, 1, rate, 0.0)]
    for name, db in P.VOLUMES_DB.items():
        assert P.parse_markup('<prosody volume="{}">x</prosody>'.format(name))[1] == [(0, 1, 1.0, db)]
    for name, (rate, db) in P.EMPHASIS.items():
        assert P.parse_markup('<emphasis level="{}">x</emphasis>'.format(name))[1] == [(0, 1, rate, db)]
    assert P.parse_markup('<emphasis>x</emphasis>')[1] == [(0, 1) + P.EMPHASIS['moderate']]
    assert P.parse_markup('<prosody rate="0.8">x</prosody><prosody rate="120%">y</prosody>')[1] == [(0, 1, 0.8, 0.0), (1, 2, 1.2, 0.0)]
    assert sorted(P.RATES) == sorted(['x-slow', 'slow', 'medium', 'fast', 'x-fast']) and P.RATES['medium'] == 1.0
    assert sorted(P.VOLUMES_DB) == sorted(['silent', 'x-soft', 'soft', 'medium', 'loud', 'x-loud']) and P.VOLUMES_DB['medium'] == 0.0
    # breaks by time and by strength: the pause table of synthesize_text
    assert P.parse_markup('a<break time="1.5s"/>b<break time="20ms"/>')[2] == [(1, 1500.0), (2, 20.0)]
    want = {'none': 0.0, 'x-weak': 0.0, 'weak': inf.PAUSES_MS['clause'], 'medium': inf.PAUSES_MS['sentence'], 'strong': inf.PAUSES_MS['sentence'],
            'x-strong': inf.PAUSES_MS['paragraph']}
    for name, ms in want.items():
        assert P.parse_markup('a <break strength="{}"/>b'.format(name))[2] == [(2, ms)]
    assert P.parse_markup('a<break/>')[2] == [(1, inf.PAUSES_MS['sentence'])]
    assert P.parse_markup('a<break strength="weak"/>', {'clause': 50.0})[2] == [(1, 50.0)]
    # the root
    assert P.parse_markup(' <speak>Hi <break time="5ms"/>there</speak>\n') == ('Hi there', [], [(3, 5.0)])
    assert P.parse_markup('<speak/>') == ('', [], [])


def test_parse_markup_refuses_with_the_thing_and_its_offset():
    P = pkg('tacotron.prosody')
    for text, words in (
            ('ab <foo>c</foo>', ('unknown element <foo>', 'offset 3')),
            ('ab <prosody pitch="high">c</prosody>', ('unknown attribute pitch=', '<prosody>', 'offset 3')),
            ('<emphasis rate="2">c</emphasis>', ('unknown attribute rate=', '<emphasis>', 'offset 0')),
            ('a<break length="1s"/>', ('unknown attribute length=', '<break>', 'offset 1')),
            ('<speak version="1.0">a</speak>', ('unknown attribute version=', '<speak>', 'offset 0')),
            ('ab <prosody rate="quick">c</prosody>', ("rate='quick'", 'offset 3')),
            ('<prosody rate="-50%">c</prosody>', ("rate='-50%'", 'offset 0')),
            ('<prosody rate="0">c</prosody>', ("rate='0'", 'offset 0')),
            ('abc <prosody volume="6dB">c</prosody>', ("volume='6dB'", 'offset 4')),
            ('<prosody volume="loudest">c</prosody>', ("volume='loudest'", 'offset 0')),
            ('<emphasis level="none">c</emphasis>', ("level='none'", 'offset 0')),
            ('a <break time="3 ms"/>', ("time='3 ms'", 'offset 2')),
            ('a <break time="61s"/>', ("time='61s'", 'offset 2')),
            ('a <break strength="huge"/>', ("strength='huge'", 'offset 2')),
            ('a <break time="1s" strength="weak"/>', ('both time= and strength=', 'offset 2')),
            ('a <break>b</break>', ('<break>', 'must be empty')),
            ('a <prosody rate="50%">b', ('malformed markup', 'offset 23')),
            ('a </prosody> b', ('malformed markup', 'offset 4', 'mismatched tag')),         # (the parser's own position: inside the tag)
            ('a <prosody rate="50%">b</emphasis>', ('malformed markup', 'offset 25', 'mismatched tag')),
            ('a & b', ('malformed markup', 'offset 3')),
            ('a < b', ('malformed markup', 'offset 3')),
            ('x <speak>a</speak>', ('<speak>', 'offset 2', 'not the root')),
            ('<speak>a</speak> b', ('text', 'outside <speak>')),
            ('<speak>a</speak><break/>', ('<break>', 'offset 16', 'outside <speak>')),
            ('<speak><speak>a</speak></speak>', ('<speak>', 'offset 7', 'not the root'))):
        with pytest.raises(ValueError) as e:
            P.parse_markup(text)
        assert str(e.value).startswith('parse_markup: ') and all(w in str(e.value) for w in words), (text, str(e.value))
    with pytest.raises(ValueError):
        P.parse_markup(b'bytes')


# ---------------------------------------------------------------------------------------------- token_attributes
def test_token_attributes_through_the_abbreviations():
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    ds = _dataset()
    one = (65536, np.float32(1.0))
    # the expansion of an abbreviation belongs to the span that holds the abbreviation
    plain, spans, breaks = P.parse_markup('See <prosody rate="50%" volume="-6 dB">Mr. Jones</prosody> now.')
    processed, _tok = M.token_spans(ds, plain)
    assert processed == 'see mister jones now'                                                                        # (the front end drops the full stop)
    attrs, tb = P.token_attributes(ds, plain, spans, breaks)
    slow = (32768, np.float32(10.0 ** (-6.0 / 20.0)))
    assert len(attrs) == len(processed) + 1 and tb == []
    assert attrs[:4] == [one] * 4 and attrs[4:16] == [slow] * 12 and attrs[16:] == [one] * 5                          # 'mister jones'; the end token: base
    assert attrs[4][1].dtype == np.float32
    # a span that ends inside an abbreviation does not reach its expansion; the base rate multiplies
    plain, spans, breaks = P.parse_markup('<prosody rate="2">See M</prosody>r. Jones<break time="200ms"/>')
    attrs, tb = P.token_attributes(ds, plain, spans, breaks, 1.25, HOP, SR)
    fast, base = (int(65536 * 2.5), np.float32(1.0)), (81920, np.float32(1.0))
    assert attrs[:4] == [fast] * 4 and attrs[4:] == [base] * (len(attrs) - 4)
    assert tb == [(len(attrs) - 1, 16)]                                                                               # in front of the end token: 200 ms = 16.04 frames
    # breaks: in front of the first token at or behind them, inside an abbreviation behind its expansion, two at one token add up
    plain, spans, breaks = P.parse_markup('<break time="100ms"/>M<break time="100ms"/>r. J<break time="1ms"/><break time="12.5ms"/>o<break strength="none"/>')
    attrs, tb = P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR)
    assert tb == [(0, 8), (6, 8), (8, 2)] and P.break_frames(0.0, HOP, SR) == 0 and P.break_frames(1.0, HOP, SR) == 1
    # a product of rates outside [0.25, 4], a gain above 16: the span is named
    plain, spans, breaks = P.parse_markup('a <prosody rate="x-slow"><prosody rate="40%">bc</prosody></prosody>')
    with pytest.raises(ValueError) as e:
        P.token_attributes(ds, plain, spans, breaks)
    assert "span 1 ('bc', characters 2 .. 4)" in str(e.value) and '[0.25, 4]' in str(e.value)
    with pytest.raises(ValueError) as e:
        P.token_attributes(ds, plain, spans, breaks, 0.4)
    assert "span 0 ('bc', characters 2 .. 4)" in str(e.value)
    P.token_attributes(ds, plain, spans[:1], breaks, 0.5)
    plain, spans, breaks = P.parse_markup('<prosody volume="+24 dB">a</prosody><prosody volume="+25 dB">b</prosody>')
    with pytest.raises(ValueError) as e:
        P.token_attributes(ds, plain, spans, breaks)
    assert "span 1 ('b', characters 1 .. 2)" in str(e.value) and 'gain above 16' in str(e.value)
    assert P.volume_gain(-math.inf) == 0.0 and P.volume_gain(0.0) == 1.0
    for bad in (0.2, 4.5, float('nan')):
        with pytest.raises(ValueError):
            P.token_attributes(ds, 'a', [], [], bad)


# ---------------------------------------------------------------------------------------------- segments_of_row, warp_position
ONE, SLOW, LOUD = (65536, 1.0), (32768, 1.0), (65536, 2.0)


def test_segments_of_row_on_hand_made_starts():
    P = pkg('tacotron.prosody')
    #        tokens: 0  1  2  3  4  5(end)   token 2 has no step
    start = [0, 2, 3, 3, 6, 8, 9, 9]          # (Ts + 1 = 8 entries; behind n_sent = 6: the steps)
    attrs = [ONE, ONE, SLOW, SLOW, LOUD, ONE]
    seg, n_out = P.segments_of_row(start, 6, R, 45, attrs, [], 1, row=2)
    assert seg == [(2, 0, 15, 0, 65536, 1.0), (2, 15, 15, 0, 32768, 1.0), (2, 30, 10, 0, 65536, 2.0), (2, 40, 5, 0, 65536, 1.0)]   # merged, skipped
    assert n_out == 15 + 30 + 10 + 5
    # the end-of-speech clip: a token cut short, tokens cut away
    seg, n_out = P.segments_of_row(start, 6, R, 33, attrs, [], 1)
    assert seg == [(0, 0, 15, 0, 65536, 1.0), (0, 15, 15, 0, 32768, 1.0), (0, 30, 3, 0, 65536, 2.0)] and n_out == 48
    seg, n_out = P.segments_of_row(start, 6, R, 7, attrs, [], 1)
    assert seg == [(0, 0, 7, 0, 65536, 1.0)] and n_out == 7
    # breaks: in front of token 0, in front of a skipped token, in front of the end token; behind the cut: at the end
    seg, n_out = P.segments_of_row(start, 6, R, 45, attrs, [(0, 4), (2, 3), (5, 2)], 1)
    assert seg == [(0, 0, 0, 4, 0, 0.0), (0, 0, 15, 0, 65536, 1.0), (0, 0, 0, 3, 0, 0.0), (0, 15, 15, 0, 32768, 1.0), (0, 30, 10, 0, 65536, 2.0),
                   (0, 0, 0, 2, 0, 0.0), (0, 40, 5, 0, 65536, 1.0)]
    assert n_out == 69
    seg, n_out = P.segments_of_row(start, 6, R, 20, attrs, [(4, 3), (5, 2)], 1)
    assert seg == [(0, 0, 15, 0, 65536, 1.0), (0, 15, 5, 0, 32768, 1.0), (0, 0, 0, 5, 0, 0.0)] and n_out == 30                      # pauses that meet are one
    # a break splits what would merge
    seg, _n = P.segments_of_row(start, 6, R, 45, [ONE] * 6, [(1, 1)], 1)
    assert seg == [(0, 0, 10, 0, 65536, 1.0), (0, 0, 0, 1, 0, 0.0), (0, 10, 35, 0, 65536, 1.0)]
    # the padding to min_frames
    seg, n_out = P.segments_of_row(start, 6, R, 2, [(262144, 1.0)] * 6, [], 4)
    assert seg == [(0, 0, 2, 0, 262144, 1.0), (0, 0, 0, 3, 0, 0.0)] and n_out == 4
    seg, n_out = P.segments_of_row(start, 6, R, 2, [(262144, 1.0)] * 6, [(5, 1)], 4)
    assert seg == [(0, 0, 2, 0, 262144, 1.0), (0, 0, 0, 3, 0, 0.0)] and n_out == 4
    # sum(count) == n_out of the oracle's plan, and of the library's
    rng = np.random.default_rng(11)
    H = pkg('_hip')
    for _ in range(50):
        n_sent = int(rng.integers(1, 12))
        steps = np.sort(rng.integers(0, 9, n_sent - 1)).tolist()
        start = [0] + steps + [8] + [8] * 3
        attrs = [(int(rng.integers(O.STEP_MIN, O.STEP_MAX + 1)), float(np.float32(rng.random() * 3))) if rng.random() < 0.7 else ONE for _j in range(n_sent)]
        breaks = [(int(j), int(rng.integers(1, 9))) for j in range(n_sent) if rng.random() < 0.3]
        n_frames = int(rng.integers(1, 41))
        seg, n_out = P.segments_of_row(start, n_sent, R, n_frames, attrs, breaks, 6)
        why, want, counts = O.plan(seg, 1, 40, [n_frames])
        assert why is None and want == [n_out] == [sum(counts)] and n_out >= 6
        assert H.warp_list(seg, 1, 40, [n_frames])[2].tolist() == [n_out]
        speech = [q for q in seg if q[2]]
        assert speech[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(speech[:-1], speech[1:]))              # contiguous from frame 0
        assert speech[-1][1] + speech[-1][2] == min(n_frames, 40)
        assert all(not (a[2] == 0 and b[2] == 0) for a, b in zip(seg[:-1], seg[1:]))                                 # no two pauses meet
    for bad in (dict(start=[0, 1], n_sent=2), dict(attrs=[ONE]), dict(n_frames=0), dict(breaks=[(6, 1)]), dict(breaks=[(0, 0)])):
        kw = dict(dict(start=[0, 2, 3, 3, 6, 8, 9, 9], n_sent=6, r=R, n_frames=5, attrs=[ONE] * 6, breaks=[]), **bad)
        with pytest.raises(ValueError):
            P.segments_of_row(kw['start'], kw['n_sent'], kw['r'], kw['n_frames'], kw['attrs'], kw['breaks'])


def test_warp_position_at_the_borders():
    P = pkg('tacotron.prosody')
    seg = [(0, 0, 0, 4, 0, 0.0), (0, 0, 15, 0, 65536, 1.0), (0, 15, 15, 0, 32768, 1.0), (0, 0, 0, 3, 0, 0.0), (0, 30, 10, 0, 98304, 2.0), (0, 0, 0, 2, 0, 0.0)]
    n_out = 4 + 15 + 30 + 3 + 7 + 2                     # (10 frames at 1.5: ceil(6.67) = 7)
    pos = P.warp_position
    assert pos(seg, 0) == 4.0 and pos(seg, 0, 'left') == 0.0                                   # a pause in front of the first frame
    assert pos(seg, 15) == pos(seg, 15, 'left') == 19.0                                       # continuous from one speech segment into the next
    assert pos(seg, 7.5) == 11.5 and pos(seg, 20) == 29.0 and pos(seg, 22.5) == 34.0
    assert pos(seg, 30, 'left') == 49.0 and pos(seg, 30) == 52.0                              # across a pause: its frames apart
    assert pos(seg, 35) == 52.0 + 3.5 and pos(seg, 40, 'left') == 59.0
    assert pos(seg, 40) == pos(seg, 1000) == float(n_out) == 61.0                              # it ends at n_out
    xs = np.linspace(0.0, 40.0, 801)
    for side in ('right', 'left'):
        ys = [pos(seg, x, side) for x in xs]
        assert all(b >= a for a, b in zip(ys[:-1], ys[1:]))                                   # monotone
    ys = [pos(seg, x) for x in xs]
    big = [round(float(x), 2) for x, a, b in zip(xs[1:], ys[:-1], ys[1:]) if b - a > 0.11]
    assert big == [30.0, 40.0]                                                                # continuous except across a pause (steps of 0.05 frames move at most 0.1)
    with pytest.raises(ValueError):
        pos(seg, 1.0, 'middle')
    assert pos([], 3.0) == 0.0


# ---------------------------------------------------------------------------------------------- the marks
def _marks(P, M, ds, marked, start, n_frames, min_frames=1):
    plain, spans, breaks = P.parse_markup(marked)
    processed, tok = M.token_spans(ds, plain)
    attrs, tb = P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR)
    seg, n_out = P.segments_of_row(start, len(processed) + 1, R, n_frames, attrs, tb, min_frames)
    place = lambda x: HOP * P.warp_position(seg, x / HOP, 'right')
    place_end = lambda x: HOP * P.warp_position(seg, x / HOP, 'left')
    marks = M.marks_of_row(processed, tok, start, R, HOP, 1.0, HOP * (n_frames - 1), SR, None, HOP * (n_out - 1), 'word', raw=plain,
                           place=place, place_end=place_end)
    return marks, seg, n_out


def test_the_marks_of_a_slowed_word_and_of_a_break():
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    ds = _dataset()
    #             o  n  e  _  t  w  o  _  s  i  x  end
    start = [0, 1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14]
    n_frames = 70
    plain_marks, seg, n_out = _marks(P, M, ds, 'one two six', start, n_frames)
    assert seg == [(0, 0, 70, 0, 65536, 1.0)] and n_out == 70
    # ... the unmarked marks are marks_of_row's own
    assert plain_marks == M.marks_of_row('one two six', [(i, i + 1) for i in range(11)], start, R, HOP, 1.0, HOP * 69, SR, None, HOP * 69, 'word', raw='one two six')
    slow_marks, seg, n_out = _marks(P, M, ds, 'one <prosody rate="50%">two</prosody> six', start, n_frames)
    assert seg == [(0, 0, 20, 0, 65536, 1.0), (0, 20, 25, 0, 32768, 1.0), (0, 45, 25, 0, 65536, 1.0)] and n_out == 95
    words = lambda marks: [m for m in marks if m['type'] == 'word']
    a, b = words(plain_marks), words(slow_marks)
    assert [m['value'] for m in b] == ['one', 'two', 'six'] and [(m['start'], m['end']) for m in b] == [(0, 3), (4, 7), (8, 11)]
    assert b[0] == a[0]
    # exactly twice in samples; the milliseconds are each one rounding of 1000 * samples / rate, so their differences agree to a few ulp
    near = lambda v: pytest.approx(v, rel=1e-12, abs=0.0)
    assert b[1]['end_sample'] - b[1]['sample'] == 2 * (a[1]['end_sample'] - a[1]['sample']) == 2 * 25 * HOP and b[1]['sample'] == a[1]['sample']
    assert b[1]['end_ms'] - b[1]['time_ms'] == near(2.0 * (a[1]['end_ms'] - a[1]['time_ms'])) and b[1]['time_ms'] == a[1]['time_ms']
    grown = 1000.0 * 25 * HOP / SR
    for x, y in zip(a[2:], b[2:]):                                                             # every later mark is shifted by the difference
        assert y['time_ms'] == near(x['time_ms'] + grown) and y['end_ms'] == near(x['end_ms'] + grown)
        assert y['sample'] == x['sample'] + 25 * HOP and y['end_sample'] == x['end_sample'] + 25 * HOP
    # a 300 ms break: 24 frames between the neighbouring words' marks (the blank in front of 'six' has no step here)
    start2 = [0, 1, 2, 3, 4, 6, 7, 9, 9, 11, 12, 13, 14]
    c = words(_marks(P, M, ds, 'one two six', start2, n_frames)[0])
    brk, seg, n_out = _marks(P, M, ds, 'one two <break time="300ms"/>six', start2, n_frames)
    d = words(brk)
    frames = P.break_frames(300.0, HOP, SR)
    assert frames == 24 and (0, 0, 0, 24, 0, 0.0) in seg and n_out == 94
    assert c[2]['time_ms'] - c[1]['end_ms'] == 0.0
    assert d[2]['time_ms'] - d[1]['end_ms'] == near(1000.0 * frames * HOP / SR)
    assert d[:2] == c[:2] and d[2]['sample'] - d[1]['end_sample'] == frames * HOP
    # ... and with steps for the blank the gap grows by exactly the pause
    e = words(_marks(P, M, ds, 'one two <break time="300ms"/>six', start, n_frames)[0])
    assert (e[2]['sample'] - e[1]['end_sample']) - (a[2]['sample'] - a[1]['end_sample']) == frames * HOP
    assert (e[2]['time_ms'] - e[1]['end_ms']) - (a[2]['time_ms'] - a[1]['end_ms']) == pytest.approx(1000.0 * frames * HOP / SR, rel=1e-9)


# ---------------------------------------------------------------------------------------------- inference
def test_synthesize_marked_refuses_before_it_touches_an_engine():
    inf = pkg('tacotron.inference')
    model = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params)     # no engine: touching it is an AttributeError
    ds = _dataset()
    for kw in (dict(pitch=0.5), dict(momentum=2.0), dict(speaking_rate=9.0), dict(phase_init='guess'), dict(loudness=float('nan')),
               dict(marks='syllable'), dict(output='mp3')):
        with pytest.raises(ValueError):
            inf.synthesize_marked(model, ['A text.'], ds, **kw)
    for bad in (['A <b>bold</b> text.'], ['<prosody rate="x-slow"><prosody rate="30%">too slow</prosody></prosody>'], []):
        with pytest.raises(ValueError):
            inf.synthesize_marked(model, bad, ds)
    with pytest.raises(ValueError):
        inf.synthesize_marked(model, ['<prosody rate="50%">slow</prosody>'], ds, speaking_rate=0.4)


def test_the_command_line_parses():
    inf = pkg('tacotron.inference')
    assert inf.parse_args([]).markup is False
    args = inf.parse_args(['--markup', '--marks', '--rate', '1.2'])
    assert (args.markup, args.marks, args.rate, args.text, args.pitch) == (True, 'word', 1.2, False, 0.0)
    for bad in (['--markup', '--text'], ['--markup', '--pitch', '2']):
        with pytest.raises(SystemExit) as e:
            inf.parse_args(bad)
        assert e.value.code == 2
    assert '--markup' in inf.main.__doc__
