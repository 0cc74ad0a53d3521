"""Host side of per-word pitch, no GPU: tests/resample_segments_oracle.py against tests/resample_oracle.py (one segment is the
uniform resampler), the binding's checks against the oracle's, and the planner of tacotron/prosody.py -- pitch parsing and its
refusals, the quarter-semitone grid, steps and ratios, the merge into sample segments, ``pitch_position`` -- up to the options
of ``synthesize_marked`` and the command line."""
import math
import types

import numpy as np
import pytest

import resample_cases as RC
import resample_oracle as R
import resample_segments_cases as C
import resample_segments_oracle as O
from conftest import pkg
from host_checks import no_device_engine

HOP, SR, RED = 275, 22050, 5


def _dataset():
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)


def test_symbols():
    H = pkg('_hip')
    assert H.RESAMPLE_SEGMENT.itemsize == 24 == __import__('ctypes').sizeof(H.TtsResampleSegment)
    assert [H.RESAMPLE_SEGMENT.fields[k][1] for k in ('row', 'first', 'samples', 'reserved', 'ratio')] == [0, 4, 8, 12, 16]
    assert (H.RESAMPLE_SEGMENTS_MAX, H.RESAMPLE_SEGMENTS_PER_LAUNCH, H.RESAMPLE_SEGMENTS_MAX_RATIOS) == (O.MAX_SEGMENTS, O.SEGMENTS_PER_LAUNCH, O.MAX_RATIOS)
    for name in ('tts_resample_segments_plan', 'tts_resample_segments', 'tts_resample_segments_max', 'tts_resample_segments_max_ratios',
                 'tts_resample_segments_tile'):
        assert name in H._PROTOTYPES
    header = open(__import__('os').path.join(__import__('conftest').ROOT, 'include', 'sstts_hip.h')).read()
    assert 'tts_resample_segment_t' in header and 'int tts_resample_segments_tile(void);' in header


@pytest.mark.parametrize('rho', [r for r in RC.RATIOS if r != 1.0], ids=[i for i in RC.RATIO_IDS if i != '1.0'])
def test_one_segment_is_the_uniform_resampler(rho):
    """(b, 0, n_b, ratio) per row: y and sabs of resample_oracle.resample, bit for bit, and the zeros behind them"""
    x = RC.ragged_batch()
    want_y, want_s = RC.oracle('ragged', rho)
    N_out = want_y.shape[1]
    got = O.resample_segments(x, [(b, 0, n, rho) for b, n in enumerate(RC.RAGGED)], RC.RAGGED, N_out)
    assert got['n_out'] == [R.resampled_valid(n, rho) for n in RC.RAGGED]
    assert np.array_equal(got['y'], want_y) and np.array_equal(got['sabs'], want_s)
    for b, n in enumerate(RC.RAGGED):
        k = got['n_out'][b]
        assert (got['kind'][b, :k] == O.RESAMPLED).all() and not got['kind'][b, k:].any() and not got['bits'][b, k:].any()
        if k:                                                                                   # the windows the oracle reports are resample_oracle's
            for src in (0, n // 2, n - 1):
                assert np.array_equal((got['lo'][b, :k] <= src) & (src <= got['hi'][b, :k]), R.covers(n, rho, src))


def test_the_oracles_layout_copies_and_first():
    x = C.batch()
    case = C.mixed()
    got = C.oracle('mixed', 3)
    why, n_out, counts = O.plan(case['segments'], 6, C.N, case['n_samples'])
    assert why is None and got['n_out'] == n_out == [sum(c for q, c in zip(case['segments'], counts) if q[0] == b) for b in range(6)]
    # a copy is the source's bits; a segment from `first` is the whole-row resampling of the row shifted by first -- where no window is cut
    o = sum(counts[12:13])
    assert np.array_equal(got['bits'][4, :o], x[4, 100:355].view(np.uint32)) and (got['kind'][4, :o] == O.COPY).all()
    row = np.nan_to_num(x[5, :5000].astype(np.float64))
    first, samples, rho = 1000, 3000, RC.RATIOS[2]
    y, s, lo, hi = O.segment(row, first, O.count(samples, rho), rho)
    y0, s0 = R.resample(row[first:], rho)
    taps = R.NWIN // R.consts(rho)[1] + 1
    inner = slice(int(taps * rho) + 2, len(y))
    assert np.array_equal(y[inner], y0[:len(y)][inner]) and np.array_equal(s[inner], s0[:len(y)][inner])
    assert not np.array_equal(y[:8], y0[:8])                                                    # ... and at the border the taps reach into the row
    assert lo[0] == first - taps + 1 + 1 or lo[0] == first - taps + 1                           # (off = 0: 32769 // step taps)
    assert hi[-1] > first + samples - 1 or samples * rho != int(samples * rho)


def _lists():
    ok = C.mixed()['segments']
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(ok)]
    yield ok, 6, list(RC.RAGGED)
    yield [], 6, None
    yield ok, 0, None
    yield [(0, 0, 1, 1.0)] * 4097, 1, None
    yield ok, 29, None
    yield ok, 6, [1, 2, 63, 64, 5001, 5000]
    yield edit(0, 0, 1), 6, None
    yield edit(7, 0, 1), 6, None
    yield [q for q in ok if q[0] != 3], 6, None
    yield [q for q in ok if q[0] != 5], 6, None
    yield edit(13, 2, 0), 6, list(RC.RAGGED)
    yield edit(13, 2, 513), 6, list(RC.RAGGED)
    yield edit(13, 1, -1), 6, list(RC.RAGGED)
    for v in (0.2, 4.5, float('nan'), float('inf'), -1.0):
        yield edit(13, 3, v), 6, list(RC.RAGGED)
    yield [(0, 0, 10, 2.0 ** (-(k + 1) / 48.0)) for k in range(17)], 1, None
    yield [(0, 0, 10, 2.0 ** (-(k + 1) / 48.0)) for k in range(16)] + [(0, 0, 10, 1.5), (0, 0, 10, 1.0)], 1, None


def test_the_python_checks_are_the_oracles():
    H = pkg('_hip')
    legal = 0
    for seg, B, ns in _lists():
        why, n_out, counts = O.plan(seg, B, C.N, ns)
        if why is None:
            q, got_ns, got_n, got_c = H.resample_segment_list(seg, B, C.N, ns)
            assert q.dtype == H.RESAMPLE_SEGMENT and got_n.tolist() == n_out and got_c.tolist() == counts and not q['reserved'].any()
            legal += 1
        else:
            with pytest.raises(ValueError) as e:
                H.resample_segment_list(seg, B, C.N, ns)
            text = str(e.value)
            assert text == ('resample_segments: ' + why if not why.startswith('n_samples[') else why), (text, why)
    assert legal == 2
    # reserved travels only in a RESAMPLE_SEGMENT array
    q = C.segment_array(H, [(0, 0, 5, 0.5, 3)])
    with pytest.raises(ValueError, match='segment 0 has reserved = 3, which must be 0'):
        H.resample_segment_list(q, 1, 10)
    for bad in ([(0, 0, 5)], [(0, 0.5, 5, 1.0)], [(0, 0, 5, 'x')], 7, [(0, 0, 2 ** 31, 1.0)]):
        with pytest.raises(ValueError):
            H.resample_segment_list(bad, 1, 10)
    # the engine's methods refuse before they touch a handle
    eng = no_device_engine()
    x = np.zeros((1, 10), np.float32)
    for call in (lambda: eng.resample_segments(x, [(0, 0, 11, 0.5)]), lambda: eng.resample_segments(x, [(0, 0, 10, 0.5)], N_out=4),
                 lambda: eng.resample_segments(x[0], [(0, 0, 10, 0.5)]), lambda: eng.resample_segments_plan((1, 10, 1), [(0, 0, 10, 0.5)]),
                 lambda: eng.resample_segments(x, [(0, 0, 10, 0.5)], n_samples=[11]), lambda: eng.resample_segments_plan((1, 10), [(0, 0, 10, 9.0)])):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------- the planner
def test_parse_markup_takes_a_pitch_only_when_asked():
    P = pkg('tacotron.prosody')
    with pytest.raises(ValueError, match=r'unknown attribute pitch= of <prosody> at offset 2'):
        P.parse_markup('a <prosody pitch="+2st">b</prosody>')
    assert P.parse_markup('a <prosody rate="50%">b</prosody>') == ('a b', [(2, 3, 0.5, 0.0)], [])                # four elements, as before
    assert P.parse_markup('a <prosody rate="50%">b</prosody>', pitch=True) == ('a b', [(2, 3, 0.5, 0.0, 0.0)], [])
    table = [('+2st', 2.0), ('-3.5st', -3.5), ('+12st', 12.0), ('-12st', -12.0), ('x-low', -4.0), ('low', -2.0), ('medium', 0.0), ('high', 2.0),
             ('x-high', 4.0), ('+100%', 12.0), ('-50%', -12.0), ('+0%', 0.0), ('+5.95%', 1.0), ('+0.3st', 0.25), ('+0.38st', 0.5), ('-0.12st', 0.0),
             ('-0.125st', -0.25), ('+0.125st', 0.25), ('+12.1st', 12.0)]
    for value, st in table:
        _plain, spans, _b = P.parse_markup('<prosody pitch="{}">x</prosody>'.format(value), pitch=True)
        assert spans == [(0, 1, 1.0, 0.0, st)], value
    # nested pitches add before the rounding; emphasis keeps its meaning and the pitch around it; rate and volume travel beside it
    plain, spans, breaks = P.parse_markup('<speak>a <prosody pitch="+0.6st" rate="80%">b <prosody pitch="+0.6st" volume="-6 dB">c <emphasis>d</emphasis>'
                                          '</prosody></prosody> <prosody pitch="low">e<break time="1s"/></prosody></speak>', pitch=True)
    assert plain == 'a b c d e' and breaks == [(9, 1000.0)]
    assert spans == [(2, 7, 0.8, 0.0, 0.5), (4, 7, 0.8, -6.0, 1.25), (6, 7, 0.8 * 0.9, -6.0 + 1.5, 1.25), (8, 9, 1.0, 0.0, -2.0)]
    assert P.round_semitones(0.6) == 0.5 and P.round_semitones(1.2) == 1.25 and P.round_semitones(-0.0) == 0.0 and P.round_semitones(-0.37) == -0.25
    for bad, what, at in [('a <prosody pitch="200Hz">b</prosody>', "pitch='200Hz' at offset 2", 2), ('<prosody pitch="+13st">x</prosody>', '+13 semitones', 0),
                          ('<prosody pitch="+7st">x <prosody pitch="+6st">y</prosody></prosody>', "pitch='+6st' at offset 24", 24),
                          ('<prosody pitch="-12.2st">x</prosody>', '-12.25 semitones', 0), ('<prosody pitch="2st">x</prosody>', "pitch='2st'", 0),
                          ('<prosody pitch="-100%">x</prosody>', "pitch='-100%'", 0), ('<prosody pitch="loud">x</prosody>', "pitch='loud'", 0),
                          ('ab <prosody pitch="">x</prosody>', "pitch=''", 3)]:
        with pytest.raises(ValueError) as e:
            P.parse_markup(bad, pitch=True)
        assert what in str(e.value) and 'offset {}'.format(at) in str(e.value), (bad, str(e.value))
    assert 'Hz is not supported' in str(pytest.raises(ValueError, P.parse_markup, '<prosody pitch="+20Hz">x</prosody>', pitch=True).value)
    assert 'UNTUNED' in P.__doc__ and 'pitch' in P.__doc__


def test_token_attributes_with_a_pitch():
    P = pkg('tacotron.prosody')
    ds = _dataset()
    plain, spans, breaks = P.parse_markup('one <prosody pitch="+4st" rate="80%">two</prosody> <prosody pitch="-12st">six</prosody>', pitch=True)
    attrs, tb = P.token_attributes(ds, plain, spans, breaks, 1.25, HOP, SR, pitch=True)
    up, down = 2.0 ** (-4.0 / 12.0), 2.0 ** (12.0 / 12.0)
    assert tb == [] and len(attrs) == 12 and all(len(a) == 3 for a in attrs)
    assert attrs[0] == (81920, np.float32(1.0), 1.0) == attrs[3] == attrs[7] == attrs[11]
    assert attrs[4] == attrs[6] == (int(math.floor(65536 * 1.25 * 0.8 * up + 0.5)), np.float32(1.0), up) and attrs[4][0] == 52016
    assert attrs[8] == attrs[10] == (163840, np.float32(1.0), down) and down == 2.0
    # without a pitch in the text the steps are those of the call without the option, and every ratio is 1.0
    plain, spans, breaks = P.parse_markup('one <prosody rate="80%">two</prosody> six')
    old, _tb = P.token_attributes(ds, plain, spans, breaks, 1.25, HOP, SR)
    new, _tb = P.token_attributes(ds, *P.parse_markup('one <prosody rate="80%">two</prosody> six', pitch=True), 1.25, HOP, SR, pitch=True)
    assert [a[:2] for a in new] == old and {a[2] for a in new} == {1.0} and all(len(a) == 2 for a in old)
    # a step outside 16384 .. 262144 names the span
    for marked, base in (('<prosody pitch="+12st" rate="40%">slow</prosody>', 1.0), ('a <prosody pitch="-12st">b</prosody>', 2.5)):
        with pytest.raises(ValueError, match=r'token_attributes: span 0 \(.*the step \d+ is not in 16384 \.\. 262144'):
            P.token_attributes(ds, *P.parse_markup(marked, pitch=True), base, HOP, SR, pitch=True)


def _plan(P, M, ds, marked, start, n_frames, pitch=True):
    plain, spans, breaks = P.parse_markup(marked, pitch=pitch)
    processed, tok = M.token_spans(ds, plain)
    attrs, tb = P.token_attributes(ds, plain, spans, breaks, 1.0, HOP, SR, pitch=pitch)
    seg, n_out, *ratios = P.segments_of_row(start, len(processed) + 1, RED, n_frames, attrs, tb)
    return plain, processed, tok, seg, n_out, (ratios[0] if pitch else None)


START = [0, 1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14]          # o n e _ t w o _ s i x end
UP4 = 2.0 ** (-4.0 / 12.0)


def test_pitch_segments_of_row_clips_and_merges():
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    ds = _dataset()
    _pl, _pr, _tok, seg, n_out, ratios = _plan(P, M, ds, 'one <prosody pitch="+4st">two</prosody> <break time="300ms"/>six', START, 70)
    step = int(math.floor(65536 * UP4 + 0.5))
    frames = P.warp_count(25, step)
    assert seg == [(0, 0, 20, 0, 65536, 1.0), (0, 20, 25, 0, step, 1.0), (0, 45, 5, 0, 65536, 1.0), (0, 0, 0, 24, 0, 0.0), (0, 50, 20, 0, 65536, 1.0)]
    assert ratios == [1.0, UP4, 1.0, 1.0, 1.0] and n_out == 20 + frames + 5 + 24 + 20 and frames == 32
    pseg, n_new = P.pitch_segments_of_row(seg, ratios, HOP, n_out, row=3)
    # speech, the pitched word, then speech + pause + speech merged into one copy that the row's hop (n_out - 1) clips by one frame
    assert pseg == [(3, 0, 20 * HOP, 1.0), (3, 20 * HOP, frames * HOP, UP4), (3, (20 + frames) * HOP, (5 + 24 + 20 - 1) * HOP, 1.0)]
    assert n_new == 20 * HOP + int(frames * HOP * UP4) + 48 * HOP
    assert sum(q[2] for q in pseg) == HOP * (n_out - 1) and all(a[1] + a[2] == b[1] for a, b in zip(pseg, pseg[1:]))
    # a row without a pitch is one copy of itself
    _pl, _pr, _tok, seg, n_out, ratios = _plan(P, M, ds, 'one <prosody rate="50%">two</prosody> six', START, 70)
    assert P.pitch_segments_of_row(seg, ratios, HOP, n_out) == ([(0, 0, HOP * (n_out - 1), 1.0)], HOP * (n_out - 1))
    # tokens whose steps agree but whose ratios differ do not merge: 2 ** (-12 / 12) at rate 2 and no pitch at rate 1
    _pl, _pr, _tok, seg, n_out, ratios = _plan(P, M, ds, 'one <prosody pitch="+12st" rate="200%">two</prosody> six', START, 70)
    assert [q[4] for q in seg] == [65536] * 3 and ratios == [1.0, 0.5, 1.0]
    # a segment wholly behind the clip is dropped; the lists must fit each other
    assert P.pitch_segments_of_row([(0, 0, 3, 0, 65536, 1.0), (0, 3, 1, 0, 65536, 1.0)], [1.0, 0.5], HOP, 4) == ([(0, 0, 3 * HOP, 1.0)], 3 * HOP)
    for bad in (lambda: P.pitch_segments_of_row(seg, ratios[:-1], HOP, n_out), lambda: P.pitch_segments_of_row(seg, ratios, HOP, n_out + 1),
                lambda: P.pitch_segments_of_row([(0, 0, 1, 0, 65536, 1.0)], [1.0], HOP, 1)):
        with pytest.raises(ValueError):
            bad()
    # what the planner makes is a list the library takes
    why, n_rows, _c = O.plan(pseg, 4, HOP * 200, None) if False else O.plan([(0,) + q[1:] for q in pseg], 1, HOP * 200, [HOP * (20 + frames + 49 - 1)])
    assert why is None and n_rows == [n_new]


def test_pitch_position_is_monotone_continuous_and_composes_with_warp_position():
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    ds = _dataset()
    _pl, _pr, _tok, seg, n_out, ratios = _plan(P, M, ds, '<prosody pitch="-3st">one</prosody> <prosody pitch="+4st">two</prosody> <break time="300ms"/>six', START, 70)
    pseg, n_new = P.pitch_segments_of_row(seg, ratios, HOP, n_out)
    held = HOP * (n_out - 1)
    xs = np.linspace(0.0, held, 4001)
    for side in ('right', 'left'):
        ys = np.array([P.pitch_position(pseg, x, side) for x in xs])
        assert ys[0] == 0.0 and ys[-1] == n_new and (np.diff(ys) >= 0).all()
        assert np.abs(np.diff(ys)).max() <= (xs[1] - xs[0]) * 2.0 ** (3.0 / 12.0) + 1.0      # no jump: the steepest segment's slope, a sample of truncation
    for q in pseg:                                                                              # both sides agree at every border: no gap
        for x in (q[1], q[1] + q[2]):
            assert P.pitch_position(pseg, x, 'right') == P.pitch_position(pseg, x, 'left')
    assert P.pitch_position(pseg, held + 50.0) == n_new and P.pitch_position(pseg, -3.0) == 0.0
    o = 0
    for _row, first, samples, ratio in pseg:                                                    # linear inside a segment, onto what it fills
        c = O.count(samples, ratio)
        assert P.pitch_position(pseg, first + samples / 2.0) == o + c * 0.5
        o += c
    with pytest.raises(ValueError):
        P.pitch_position(pseg, 0.0, 'middle')
    # composed with warp_position: a source frame lands where its warped frame's sample lands; the break still opens a gap
    place = lambda f, side: P.pitch_position(pseg, HOP * P.warp_position(seg, f, side), side)
    fs = np.linspace(0.0, 69.0, 691)
    for side in ('right', 'left'):
        ys = [place(f, side) for f in fs]
        assert all(b >= a for a, b in zip(ys, ys[1:]))
    gap = place(50.0, 'right') - place(50.0, 'left')                                            # frame 50: where 'six' starts behind the break
    assert gap == 24 * HOP


def test_a_words_duration_with_and_without_a_pitch():
    """The retimed word lasts what it lasts without the pitch.  Per segment the resampler's count is int(samples * ratio): less
    than one sample short of samples * ratio -- the only error the pitch pass itself adds.  Where the warp's own frame count is
    exact (an octave up: step 32768; an octave down over an even number of frames: step 131072) the marks with and without the
    pitch then differ by less than one sample per segment; elsewhere the warp rounds the word up to a whole frame of the stretched spectrogram, ceil(frames * 65536 / step),
    which shows as up to hop * ratio samples more -- that frame is there without a pitch too, at every rate but 1."""
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    ds = _dataset()

    def words(marked, pitch, start=START, n_frames=70):
        plain, processed, tok, seg, n_out, ratios = _plan(P, M, ds, marked, start, n_frames, pitch)
        place = lambda x: HOP * P.warp_position(seg, x / HOP, 'right')
        place_end = lambda x: HOP * P.warp_position(seg, x / HOP, 'left')
        n_new, n_seg = HOP * (n_out - 1), 1
        if pitch:
            pseg, n_new = P.pitch_segments_of_row(seg, ratios, HOP, n_out)
            n_seg = len(pseg)
            for q in pseg:
                assert 0.0 <= q[2] * q[3] - O.count(q[2], q[3]) < 1.0
            place = lambda x, w=place: P.pitch_position(pseg, w(x), 'right')
            place_end = lambda x, w=place_end: P.pitch_position(pseg, w(x), 'left')
        marks = M.marks_of_row(processed, tok, start, RED, HOP, 1.0, HOP * (n_frames - 1), SR, None, n_new, 'word', raw=plain, place=place, place_end=place_end)
        return [m for m in marks if m['type'] == 'word'], n_seg

    plain_words, _n = words('one two six', False)
    twice = [2 * v for v in START]
    for st, start, n_frames in (('+12st', START, 70), ('-12st', twice, 140), ('+12st', twice, 140)):
        got, n_seg = words('one <prosody pitch="{}">two</prosody> six'.format(st), True, start, n_frames)
        assert n_seg == 3
        for a, b in zip(words('one two six', False, start, n_frames)[0], got):
            assert abs((b['end_sample'] - b['sample']) - (a['end_sample'] - a['sample'])) < n_seg and abs(b['sample'] - a['sample']) < n_seg
            assert abs(b['end_ms'] - a['end_ms']) < 1000.0 * n_seg / SR
    for st, ratio in (('+4st', UP4), ('-3st', 2.0 ** (3.0 / 12.0)), ('+0.25st', 2.0 ** (-0.25 / 12.0))):
        got, n_seg = words('one <prosody pitch="{}">two</prosody> six'.format(st), True)
        for a, b in zip(plain_words, got):
            d = (b['end_sample'] - b['sample']) - (a['end_sample'] - a['sample'])
            assert -n_seg < d < HOP * ratio + n_seg, (st, d)
        assert got[0] == plain_words[0]                                                         # in front of the pitch nothing moves


# ---------------------------------------------------------------------------------------------- inference
def test_synthesize_marked_refuses_before_it_touches_an_engine():
    inf = pkg('tacotron.inference')
    H = pkg('_hip')
    model = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params)     # no engine: touching it is an AttributeError
    ds = _dataset()
    with pytest.raises(ValueError, match='unknown attribute pitch='):
        inf.synthesize_marked(model, ['<prosody pitch="+2st">up</prosody>'], ds)
    with pytest.raises(ValueError, match='a pitch other than 0 is not supported with markup'):
        inf.synthesize_marked(model, ['<prosody pitch="+2st">up</prosody>'], ds, markup_pitch=True, pitch=0.25)
    with pytest.raises(ValueError, match='Hz'):
        inf.synthesize_marked(model, ['<prosody pitch="100Hz">up</prosody>'], ds, markup_pitch=True)
    with pytest.raises(ValueError, match='the step'):
        inf.synthesize_marked(model, ['<prosody pitch="+12st">up</prosody>'], ds, markup_pitch=True, speaking_rate=0.4)
    many = ' '.join('<prosody pitch="+{}st">a</prosody>'.format(0.25 * (k + 1)) for k in range(H.RESAMPLE_SEGMENTS_MAX_RATIOS + 1))
    with pytest.raises(ValueError, match='17 distinct pitches above 0'):
        inf.synthesize_marked(model, ['a b', many], ds, markup_pitch=True)
    sixteen = ' '.join('<prosody pitch="+{}st">a</prosody>'.format(0.25 * (k + 1)) for k in range(16)) + ' <prosody pitch="-2st">b</prosody>'
    with pytest.raises(AttributeError):                                             # sixteen above 0 and any number below pass the planner
        inf.synthesize_marked(model, [sixteen], ds, markup_pitch=True)
    import inspect
    assert inspect.signature(inf.synthesize_marked).parameters['markup_pitch'].default is False
    assert inspect.signature(inf.synthesize_marked_sentences).parameters['markup_pitch'].default is False


def test_the_command_line_parses():
    inf = pkg('tacotron.inference')
    assert inf.parse_args([]).markup_pitch is False and inf.parse_args(['--markup']).markup_pitch is False
    assert inf.parse_args(['--markup', '--markup-pitch', '--marks']).markup_pitch is True
    for bad in (['--markup-pitch'], ['--markup', '--markup-pitch', '--pitch', '2'], ['--markup-pitch', '--text']):
        with pytest.raises(SystemExit) as e:
            inf.parse_args(bad)
        assert e.value.code == 2
    assert '--markup-pitch' in inf.main.__doc__
