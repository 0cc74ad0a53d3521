"""Host side of the formant-preserving pitch, no GPU: the library's tts_shift_plan, the binding's shift_list and
tests/shift_oracle.py say the same of every list; the oracle's bound lets a float64 evaluation with reversed sums pass and tells a
float32 evaluation and a dropped lifter coefficient apart; special values; the listening test on the oracle (the harmonic spacing
moves, the envelope stays); and the planner of tacotron/prosody.py -- ``token_attributes(pitch_mode='envelope')`` and
``shift_segments_of_row`` -- up to the options of ``synthesize_marked`` and the command line."""
import ctypes
import os
import types

import numpy as np
import pytest

import shift_cases as C
import shift_oracle as O
from conftest import ROOT, pkg
from host_checks import no_device_engine

NAMES = ('tts_shift_magnitudes', 'tts_shift_plan', 'tts_shift_max_segments', 'tts_shift_tile', 'tts_shift_max_order')
HOP, SR, RED = 275, 22050, 5


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
        assert name in H.exported_symbols() and getattr(lib, name) is not None and name in H._PROTOTYPES
        assert 'int {}('.format(name) in header
    assert 'typedef struct tts_shift_segment' in header and '"shift"' in header
    assert lib.tts_shift_max_segments() == H.SHIFT_MAX_SEGMENTS == O.MAX_SEGMENTS == 4096
    assert lib.tts_shift_tile() == H.SHIFT_TILE == O.TILE == 8 and lib.tts_shift_max_order() == H.SHIFT_MAX_ORDER == O.MAX_ORDER == 256
    assert ctypes.sizeof(H.TtsShiftSegment) == H.SHIFT_SEGMENT.itemsize == 24
    assert [f[0] for f in H.TtsShiftSegment._fields_] == list(H.SHIFT_SEGMENT.names) == ['row', 'first', 'frames', 'reserved', 'pitch_step', 'formant_step']
    for name in ('shift_magnitudes', 'shift_plan', 'shift_max_segments', 'shift_tile'):
        assert callable(getattr(H.Engine, name))
    assert [H.shift_step(st) for st in (12, 4, 0, -4, -12)] == [O.step(st) for st in (12, 4, 0, -4, -12)] == [32768, 52016, 65536, 82570, 131072]
    assert H.shift_order(22050) == 33 and H.shift_order(16000) == 24 and H.shift_order(4000) == 8
    for bad in (12.01, -13, float('nan'), 'x'):
        with pytest.raises(ValueError):
            H.shift_step(bad)
    with open(os.path.join(ROOT, pkg().__name__, 'build.py')) as f:
        build = f.read()
    assert "'shift.hip'" in build and "'shift_plan.h'" in build and "'shift.hip': ['-fno-slp-vectorize']" in build


def _lists():
    case = C.mixed()
    seg, nf = case['segments'], case['n_frames']
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(seg)]
    ok = dict(segments=seg, B=3, F=1025, T=70, n_frames=nf, order=33)
    yield ok
    yield dict(ok, n_frames=None, segments=[q for q in seg if q != seg[7]])           # row 1 is missing
    yield dict(ok, B=0)
    yield dict(ok, T=0)
    yield dict(ok, segments=[])
    for F in (1024, 65, 4097, 1026):
        yield dict(ok, F=F)
    for order in (1, 0, -1, 257, 513):
        yield dict(ok, order=order)
    yield dict(ok, F=129, order=65)
    yield dict(ok, F=129, order=64)
    yield dict(ok, segments=[(0, s % 70, 1, 65536, 65536) for s in range(4097)], B=1, n_frames=[70])
    yield dict(ok, B=10, n_frames=[70] * 10)
    yield dict(ok, n_frames=[70, 71, 9])
    yield dict(ok, n_frames=[70, 41, 0])
    yield dict(ok, segments=edit(0, 0, 1))
    yield dict(ok, segments=edit(7, 0, 0))
    yield dict(ok, segments=seg[:-1])
    for frames in (0, -2):
        yield dict(ok, segments=edit(1, 2, frames))
    yield dict(ok, segments=edit(7, 2, 42))
    yield dict(ok, segments=edit(6, 2, 11))
    yield dict(ok, segments=edit(0, 1, -1))
    yield dict(ok, segments=edit(1, 1, 8))
    yield dict(ok, segments=edit(3, 1, 2))
    for j in (3, 4):
        for v in (32767, 131073, 0):
            yield dict(ok, segments=edit(4, j, v))
    yield dict(ok, segments=[q[:3] + (3,) + q[3:] if s == 2 else q for s, q in enumerate(seg)])
    yield dict(C.launch_seam(), F=129, order=2)
    yield dict(ok, n_frames=None)


def test_the_plan_and_every_refusal_are_the_oracles():
    """the library's tts_shift_plan, the binding's shift_list and the oracle say the same of every list, in the same words"""
    H = pkg('_hip')
    lib = H.load_library()

    def plan(segments, B, F, T, n_frames, order):
        q = C.segment_array(H, segments)
        n32 = None if n_frames is None else np.asarray(n_frames, np.int32)
        rc = lib.tts_shift_plan(q.ctypes.data if len(q) else ctypes.c_void_p(8), len(q), B, F, T,
                                None if n32 is None else n32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), order)
        return rc, (lib.tts_last_error(None) or b'').decode()

    legal, reasons = 0, set()
    for case in _lists():
        why = O.plan(**case)
        rc, text = plan(**case)
        five = all(len(q) == 5 for q in case['segments'])
        if why is None:
            legal += 1
            assert rc == H.TTS_OK, (case, text)
            q, nf = H.shift_list(case['segments'], case['B'], case['F'], case['T'], case['n_frames'], case['order'])
            assert q.dtype == H.SHIFT_SEGMENT and len(q) == len(case['segments']) and not q['reserved'].any()
            assert H.shift_list(q, case['B'], case['F'], case['T'], case['n_frames'], case['order'])[0] is not None      # (an array is taken as it is)
        else:
            reasons.add(why)
            assert rc == H.TTS_ERR_INVALID and text == 'shift_plan: ' + why, (why, text)
            with pytest.raises(ValueError) as e:
                H.shift_list(case['segments'] if five else C.segment_array(H, case['segments']), case['B'], case['F'], case['T'], case['n_frames'],
                             case['order'])
            assert str(e.value) == (why if why.startswith('n_frames[') else 'shift: ' + why), (str(e.value), why)
    assert legal == 4 and len(reasons) >= 24
    assert [H.shift_launches(S) for S in (1, 64, 65, 4096)] == [O.launches(S) for S in (1, 64, 65, 4096)] == [1, 1, 2, 64]
    assert lib.tts_shift_plan(None, 1, 1, 129, 8, None, 2) == H.TTS_ERR_INVALID
    assert (lib.tts_last_error(None) or b'').decode() == 'shift_plan: a NULL pointer (segments are required)'
    # with a NULL handle a good call and a bad one are both refused, but only the bad one with its own reason, in the documented order
    p = 4096   # any aligned non-NULL address: never dereferenced
    case = C.mixed()
    q = C.segment_array(H, case['segments'])
    pn = np.asarray(case['n_frames'], np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    lib.tts_create(None, 0, None)
    assert lib.tts_shift_magnitudes(None, p, 3, 1025, 70, pn, q.ctypes.data, len(q), 33, 2 * p) == H.TTS_ERR_INVALID
    assert not (lib.tts_last_error(None) or b'').decode().startswith('shift')
    for args, text in (((None, 3, 1025, 70, pn, q.ctypes.data, len(q), 33, p), 'a NULL pointer (mag, segments and out are required)'),
                       ((p, 0, 1025, 70, pn, q.ctypes.data, len(q), 33, p), 'out is mag: the stage does not work in place'),
                       ((p, 0, 1024, 70, pn, q.ctypes.data, len(q), 1, 2 * p), 'need B, T, S >= 1'),
                       ((p, 3, 1024, 70, pn, q.ctypes.data, len(q), 1, 2 * p), 'F = 1024 is not 2^m + 1 with 2^m in 128 .. 2048'),
                       ((p, 3, 1025, 70, pn, q.ctypes.data, 5000, 1, 2 * p), 'order = 1 is not in 2 .. 256'),
                       ((p, 3, 1025, 70, pn, q.ctypes.data, len(q), 33, 2 * p + 2), 'the buffers must be 4-byte aligned'),
                       ((p + 1, 3, 1025, 70, pn, q.ctypes.data, len(q) - 1, 33, 2 * p), 'row of segment 7 is 1: the last row is B - 1 = 2')):
        assert lib.tts_shift_magnitudes(None, *args) == H.TTS_ERR_INVALID
        assert (lib.tts_last_error(None) or b'').decode() == 'shift_magnitudes: ' + text


def test_the_python_surface_refuses_before_it_touches_a_handle():
    eng = no_device_engine()
    case = C.mixed()
    seg, nf = case['segments'], case['n_frames']
    x = np.zeros((3, 1025, 70), np.float32)
    for call in (lambda: eng.shift_magnitudes(x, seg[:-1], nf), lambda: eng.shift_magnitudes(x[0], seg, nf), lambda: eng.shift_magnitudes(x, seg, nf, order=1),
                 lambda: eng.shift_magnitudes(x, seg, nf, order=33.0), lambda: eng.shift_magnitudes(x[:, :1024], seg, nf),
                 lambda: eng.shift_magnitudes(x, seg, [70, 71, 9]), lambda: eng.shift_plan((3, 1025), seg), lambda: eng.shift_plan((3, 1025, 70), seg, nf, 600),
                 lambda: eng.shift_magnitudes(x, [(0, 0, 1, 65536)], nf), lambda: eng.shift_magnitudes(x, [(0, 0, 1, 65536, 2 ** 32)], nf),
                 lambda: eng.pitch_shift(np.zeros(4000, np.float32), 22050, 2.0, preserve_formants=True),
                 lambda: eng.pitch_shift(np.zeros(400, np.float32), 22050, 0.25, preserve_formants=True)):
        with pytest.raises(ValueError):
            call()
    E = pkg('audio.effects')
    with pytest.raises(NotImplementedError):                                   # the resampling form stays out of scope, as before
        E.pitch_shift(np.zeros(4000, np.float32), 22050, 0.25)
    with pytest.raises(ValueError):
        E.pitch_shift(np.zeros(400, np.float32), 22050, 0.25, preserve_formants=True, engine=eng)


# ---------------------------------------------------------------------------------------------- the oracle's bound
def _harmonic():
    x = C.harmonic_case()
    return x, [(0, 0, 3, C.UP4, O.UNITY)], O.shift(x, [(0, 0, 3, C.UP4, O.UNITY)], None, 33)


def test_the_bound_passes_reversed_sums_and_tells_float32_and_a_dropped_coefficient_apart():
    x, seg, res = _harmonic()
    assert res['computed'].all() and np.isfinite(res['y']).all() and (res['slack'] > 0).all()
    eta = O.eta(33, 1025, np.log(1e10))
    assert 6e-10 < eta < 8e-10 and eta < 2.0 ** -24 / 50                        # 7e-10 at Q 33, F 1025; far below float32
    # float64 with both sums reversed: within a quarter of eta (|t1| + |t2|), before any rounding to float32
    rev = O.shift(x, seg, None, 33, reverse=True)
    d = np.abs(rev['y'] - res['y'])
    assert d.max() > 0 and (d <= 0.25 * res['slack']).all()
    print('reversed sums: max |d| / slack = {:.3g}, max relative {:.3g}'.format((d / res['slack']).max(), (d / np.abs(res['y'])).max()))
    assert O.assert_holds(rev['out'].view(np.uint32), res, 'reversed') <= 1.0
    # the same arithmetic in float32: at least half of the elements break the bound
    f32 = O.shift(x, seg, None, 33, dtype=np.float32)
    over = O.excess(f32['y'].astype(np.float32), res) > 1.0
    print('float32: {:.1%} of the elements are over the bound'.format(over.mean()))
    assert over.mean() >= 0.5
    # the lifter's last coefficient dropped (h[Q - 1] c[Q - 1] is small: the raised cosine ends near zero): the bound sees it
    drop = O.shift(x, seg, None, 33, drop_last=True)
    over = O.excess(drop['out'], res) > 1.0
    print('last lifter coefficient dropped: {:.1%} over the bound'.format(over.mean()))
    assert over.mean() >= 0.5
    with pytest.raises(AssertionError):
        O.assert_holds(drop['out'].view(np.uint32), res, 'dropped')


def test_special_values():
    case = C.mixed()
    x = C.poisoned(C.with_specials(C.batch(3, 129, 70)), case['n_frames'])
    res = O.shift(x, case['segments'], case['n_frames'], 33)
    y, comp = res['out'], res['computed']
    assert comp[0, 2:9].all() and not comp[0, :2].any() and not comp[0, 17:20].any() and not comp[0, 29:34].any() and not comp[2, :3].any()
    nan = np.isnan(y)
    assert nan[0, :, 4].all() and nan[0, :, 10].all()                           # a NaN, an Inf: the whole frame, and no other
    nan[0, :, 4] = nan[0, :, 10] = False
    assert np.argwhere(nan).tolist() == [[0, 7, 30]] and y.view(np.uint32)[0, 7, 30] == 0x7fc12345   # the copied NaN keeps its payload
    assert y.view(np.uint32)[0, 8, 31] == 0x80000000                            # ... and -0.0 its sign
    assert comp[0, 22] and not y[0, :, 22].view(np.uint32).any()                # an all-zero frame: +0.0, exactly
    assert (y[0, 9:12, 37] < 0).any() and (y[0, 16:, 37] > 0).all()             # the sign follows x
    tiny = np.abs(y[0, :, 38])
    assert ((tiny > 0) & (tiny < 2.0 ** -126)).any()                            # denormals come out as denormals
    for b, n in enumerate(case['n_frames']):
        assert not y[b, :, n:].view(np.uint32).any()                            # +0.0 behind a row: the NaN there is never read
    gaps = ~comp & (np.arange(70)[None, :] < np.asarray(case['n_frames'])[:, None])
    assert np.array_equal(y.view(np.uint32)[np.broadcast_to(gaps[:, None, :], y.shape)], x.view(np.uint32)[np.broadcast_to(gaps[:, None, :], y.shape)])
    # both steps at 65536 in a computed evaluation would be x itself up to roundings: the envelope cancels
    v, _s, _m = O.shift_frames(x[1, :, :5], O.UNITY, O.UNITY, 33)
    assert np.allclose(v, x[1, :, :5], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------- the listening test, on the oracle
def _spacing(frame):
    """the harmonic spacing in Hz: the autocorrelation peak of the power spectrum over the lags for 70 .. 400 Hz"""
    p = np.asarray(frame, np.float64) ** 2
    p = p - p.mean()
    ac = np.correlate(p, p, 'full')[p.shape[0] - 1:]
    hz = C.SR / C.N_FFT
    lo, hi = int(np.ceil(70.0 / hz)), int(400.0 / hz)
    lag = lo + int(np.argmax(ac[lo:hi + 1]))
    a, b, c = ac[lag - 1], ac[lag], ac[lag + 1]
    return (lag + 0.5 * (a - c) / (a - 2.0 * b + c)) * hz


@pytest.mark.parametrize('st', [-4, 4])
def test_the_pitch_moves_and_the_envelope_stays(st):
    x = C.harmonic_case()[0]                                                    # (1025, 3): 100, 150 and 220 Hz
    N, rho = 1024, 2.0 ** (st / 12.0)
    y, _s, _m = O.shift_frames(x, O.step(st), O.UNITY, 33)
    E0, _ = O.envelope(x, 33)
    E1, _ = O.envelope(y, 33)
    i, i1, a = O.positions(N, O.step(st), False)
    moved = (1.0 - a)[:, None] * E0[i] + a[:, None] * E0[i1]                     # the envelope as a resampler would move it
    top = int(0.88 * N * min(1.0, rho))
    for c, hz in enumerate(C.TONES):
        ratio = _spacing(y[:, c]) / _spacing(x[:, c])
        kept = np.sqrt(np.mean((E1[:top, c] - E0[:top, c]) ** 2))
        resampled = np.sqrt(np.mean((moved[:top, c] - E0[:top, c]) ** 2))
        print('{:+d} st, {:g} Hz: spacing x {:.4f} (wanted {:.4f}), envelope {:.3f} nepers rms against {:.3f} resampled: {:.2f}'.format(
            st, hz, ratio, rho, kept, resampled, kept / resampled))
        assert abs(ratio / rho - 1.0) <= 0.015
        assert kept < 0.6 * resampled


# ---------------------------------------------------------------------------------------------- the planner
def test_token_attributes_in_envelope_mode():
    P = pkg('tacotron.prosody')
    ds = _dataset()
    text = 'one <prosody pitch="+4st" rate="80%">two</prosody> <prosody pitch="-12st">six</prosody>'
    plain, spans, breaks = P.parse_markup(text, pitch=True)
    env, tb = P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR, pitch=True, pitch_mode='envelope')
    none, tb0 = P.token_attributes(ds, *P.parse_markup('one <prosody rate="80%">two</prosody> six'), 1.0, HOP, SR)
    res, _tb = P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR, pitch=True)
    assert tb == tb0 and [a[:2] for a in env] == [a[:2] for a in none]          # the steps of the text without any pitch: no extra stretch
    assert [a[2] for a in env] == [0.0] * 4 + [4.0] * 3 + [0.0] + [-12.0] * 3 + [0.0]
    assert res == P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR, pitch=True, pitch_mode='resample')[0]   # the default, argument for argument
    assert [a[0] for a in res] != [a[0] for a in env] and all(len(a) == 3 for a in res)
    assert all(len(a) == 2 for a in P.token_attributes(ds, plain, [q[:4] for q in spans], breaks, 1.0, HOP, SR, pitch_mode='envelope')[0])
    with pytest.raises(ValueError, match='pitch_mode'):
        P.token_attributes(ds, plain, spans, breaks, pitch=True, pitch_mode='cepstral')
    assert P.PITCH_MODES == ('resample', 'envelope')


def test_shift_segments_of_row():
    P = pkg('tacotron.prosody')
    H = pkg('_hip')
    up, down = H.shift_step(4.0), H.shift_step(-3.0)
    # six tokens (the end token last) at steps 0, 2, 4, 6, 8, 9, 10 of r = 5 frames; a break in front of token 2
    start = [0, 2, 4, 6, 8, 9, 10]
    attrs = [(65536, 1.0, 0.0), (65536, 1.0, 4.0), (65536, 1.0, 4.0), (81920, 1.0, 4.0), (65536, 0.5, -3.0), (65536, 1.0, 0.0)]
    seg, n_out, st = P.segments_of_row(start, 6, RED, 50, attrs, [(2, 7)], row=1)
    assert [q[2] for q in seg] == [10, 10, 0, 10, 10, 5, 5] and st == [0.0, 4.0, 1.0, 4.0, 4.0, -3.0, 0.0]
    got = P.shift_segments_of_row(seg, st, 0.0, row=1)
    # the pause is skipped; tokens 1 .. 3 merge although the warp cuts them (a break, another rate): their SOURCE frames touch
    assert got == [(1, 0, 10, 65536, 65536), (1, 10, 30, up, 65536), (1, 40, 5, down, 65536), (1, 45, 5, 65536, 65536)]
    assert O.plan([(0,) + q[1:] for q in got], 1, 1025, 50, None, 33) is None
    # a timbre applies to every frame, unshifted ones too; a global pitch is the caller's sum
    tim = P.shift_segments_of_row(seg, [v + 2.0 if q[2] else 0.0 for q, v in zip(seg, st)], -1.5, row=0)
    assert [q[3:] for q in tim] == [(H.shift_step(2.0), H.shift_step(-1.5)), (H.shift_step(6.0), H.shift_step(-1.5)), (H.shift_step(-1.0), H.shift_step(-1.5)),
                                    (H.shift_step(2.0), H.shift_step(-1.5))]
    # clipped at the cut: the end-of-speech length ends the last segment, later tokens contribute nothing
    seg, n_out, st = P.segments_of_row(start, 6, RED, 33, attrs, [], row=0)
    got = P.shift_segments_of_row(seg, st, 0.0)
    assert got == [(0, 0, 10, 65536, 65536), (0, 10, 23, up, 65536)] and got[-1][1] + got[-1][2] == 33
    with pytest.raises(ValueError):
        P.shift_segments_of_row(seg, st[:-1], 0.0)
    with pytest.raises(ValueError):
        P.shift_segments_of_row(seg, [13.0] * len(seg), 0.0)
    with pytest.raises(ValueError):
        P.shift_segments_of_row(seg, st, 12.5)


def test_the_options_of_synthesize_marked_and_the_command_line():
    inf = pkg('tacotron.inference')
    assert inf.envelope_mode(True, 'envelope', -2) == (True, -2.0) and inf.envelope_mode(True, 'resample', 0.0) == (False, 0.0)
    assert inf.envelope_mode(False, 'resample', 0) == (False, 0.0)
    for args in ((False, 'envelope', 0.0), (True, 'cepstral', 0.0), (True, 'resample', 1.0), (True, 'envelope', 12.5), (True, 'envelope', float('nan')),
                 (True, 'envelope', 'x')):
        with pytest.raises(ValueError):
            inf.envelope_mode(*args)
    P = pkg('tacotron.params')
    assert inf.marked_settings(P.model_params, dict(pitch=0.25), envelope=True).octaves == 0.25
    with pytest.raises(ValueError, match='pitch'):
        inf.marked_settings(P.model_params, dict(pitch=0.25))
    model = types.SimpleNamespace(hparams=P.model_params)
    with pytest.raises(ValueError, match='markup_pitch'):
        inf.synthesize_marked(model, ['go on'], None, pitch_mode='envelope')
    with pytest.raises(ValueError, match='timbre'):
        inf.synthesize_marked(model, ['go on'], None, markup_pitch=True, timbre=1.0)
    with pytest.raises(ValueError, match='pitch'):
        inf.synthesize_marked(model, ['go on'], None, markup_pitch=True, pitch=0.25)
    ok = inf.parse_args(['--markup', '--markup-pitch', '--pitch-mode', 'envelope', '--pitch', '2', '--timbre', '-1.5'])
    assert ok.pitch_mode == 'envelope' and ok.timbre == -1.5 and ok.pitch == 2.0
    assert inf.parse_args(['--markup', '--markup-pitch']).pitch_mode == 'resample' and inf.parse_args([]).timbre == 0.0
    for bad in (['--pitch-mode', 'envelope'], ['--markup', '--pitch-mode', 'envelope'], ['--markup', '--markup-pitch', '--timbre', '1'],
                ['--markup', '--markup-pitch', '--pitch-mode', 'envelope', '--timbre', '13'], ['--markup', '--markup-pitch', '--pitch', '2'],
                ['--markup', '--markup-pitch', '--pitch-mode', 'cepstral'], ['--markup', '--markup-pitch', '--pitch-mode', 'envelope', '--text']):
        with pytest.raises(SystemExit) as e:
            inf.parse_args(bad)
        assert e.value.code == 2, bad
