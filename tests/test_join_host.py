"""Long-text synthesis without a GPU: the symbols of the join and of the speech interval; the refusals of the library and of the
Python surface made before a device is touched; the oracle's own arithmetic; ``split_text`` on a fixed table and its
properties; the pause and fade conversions, the edit list of a call and the command line of ``tacotron.inference --text``."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest

import join_oracle as O
from conftest import ROOT, pkg
from host_checks import no_device_engine

NAMES = ('tts_join', 'tts_join_plan', 'tts_join_max_pieces', 'tts_join_max_fade', 'tts_join_tile', 'tts_speech_interval')


def test_symbols():
    H = pkg('_hip')
    lib = H.load_library()
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert 'typedef struct tts_join_piece' in header and '"join"' in header
    assert lib.tts_join_max_pieces() == H.JOIN_MAX_PIECES == 4096
    assert lib.tts_join_max_fade() == H.JOIN_MAX_FADE == 1 << 20
    assert lib.tts_join_tile() == 512
    assert ctypes.sizeof(H.TtsJoinPiece) == 16 and [f[0] for f in H.TtsJoinPiece._fields_] == ['row', 'first', 'count', 'gap']
    for name in ('join', 'join_plan', 'speech_interval', 'join_max_pieces', 'join_max_fade', 'join_tile', 'download_rows'):
        assert callable(getattr(H.Engine, name))
    with open(os.path.join(ROOT, pkg().__name__, 'build.py')) as f:
        build = f.read()
    assert "'join.hip'" in build and "'join_plan.h'" in build and "'join.hip': ['-ffp-contract=off']" in build


def _list(pieces, groups):
    q = np.ascontiguousarray(pieces, dtype=np.int32).reshape(-1, 4)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    return q, g, q.ctypes.data, g.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


GOOD = ([(4, 11, 13, -6), (3, 0, 14, 2), (0, 5, 1, 0), (4, 11, 13, -1), (1, 2, 2, 1), (2, 1, 3, 9)], [0, 0, 1, 2, 2, 2])


def test_the_plan_is_the_oracles():
    H = pkg('_hip')
    lib = H.load_library()
    q, g, pq, pg = _list(*GOOD)
    n_out = np.zeros(3, np.int64)
    assert lib.tts_join_plan(pq, 6, pg, 3, 5, 2003, 7, n_out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == H.TTS_OK
    assert n_out.tolist() == O.plan(GOOD[0], GOOD[1], 7)[1] == [21, 1, 18]
    # ... and the binding's own restatement, which is what raises before the library is reached
    assert H.join_list(GOOD[0], GOOD[1], 5, 2003, 7)[3].tolist() == [21, 1, 18]
    assert H.join_list([(0, 0, 5, 3), (1, 1, 4, 0)], None, 5, 2003, 0)[2:][0] == 1
    assert H.join_fades([1, 2, 3, 13, 14, 200], 7).tolist() == O.fades([1, 2, 3, 13, 14, 200], 7) == [0, 1, 1, 6, 7, 7]


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """with a NULL handle a good call and a bad one are both refused, but only the bad one with its own reason"""
    H = pkg('_hip')
    lib = H.load_library()
    INV = H.TTS_ERR_INVALID
    p = 4096   # any aligned non-NULL address: never dereferenced

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    def join(pieces=GOOD[0], groups=GOOD[1], wav=p, B=5, N=2003, G=3, fade=7, N_out=21, out=p, P=None):
        q, g, pq, pg = _list(pieces, groups)
        return lib.tts_join(None, wav, B, N, pq if len(q) else p, len(q) if P is None else P, pg if len(g) else ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)),
                            G, fade, N_out, out)

    lib.tts_create(None, 0, None)   # (leaves its own text in the slot the refusals below must overwrite)
    assert join() == INV and not why().startswith('join')
    edit = lambda i, j, v: [tuple(v if (a, b) == (i, j) else x for b, x in enumerate(q)) for a, q in enumerate(GOOD[0])]
    for kw, text in (
            (dict(wav=None), 'join: a NULL pointer (wav, pieces, group and out are required)'),
            (dict(out=None), 'join: a NULL pointer (wav, pieces, group and out are required)'),
            (dict(B=0), 'join: need B, N, P, G >= 1'), (dict(N=0), 'join: need B, N, P, G >= 1'),
            (dict(P=0), 'join: need B, N, P, G >= 1'), (dict(G=0), 'join: need B, N, P, G >= 1'),
            (dict(fade=-1), 'join: fade < 0'),
            (dict(fade=(1 << 20) + 1), 'join: fade = 1048577 is larger than tts_join_max_fade() = 1048576'),
            (dict(P=4097), 'join: 4097 pieces are more than tts_join_max_pieces() = 4096'),
            (dict(G=7), 'join: 7 groups of 6 pieces: no group is empty'),
            (dict(G=2 ** 31 - 1), 'join: 2147483647 groups of 6 pieces: no group is empty'),      # (refused before a length is allocated)
            (dict(pieces=[(0, 0, 1, 0)] * 5, groups=[0, 1, 2, 3, 4], G=5, fade=0, N_out=2 ** 31 - 1),
             'join: G * N_out = 10737418235 output samples are more than 2^33 = 8589934592'),
            (dict(pieces=edit(2, 0, 5)), 'join: row[2] = 5 is not in 0 .. B - 1 = 4'),
            (dict(pieces=edit(1, 1, -1)), 'join: first[1] = -1 is not in 0 .. N - 1 = 2002'),
            (dict(pieces=edit(3, 2, 1993)), 'join: count[3] = 1993 is not in 1 .. N - first = 1992'),
            (dict(pieces=edit(3, 2, 0)), 'join: count[3] = 0 is not in 1 .. N - first = 1992'),
            (dict(groups=[0, 0, 2, 2, 2, 2]), 'join: group[2] = 2 follows 0: the groups are non-decreasing and none is empty'),
            (dict(groups=[0, 0, 1, 0, 0, 0]), 'join: group[3] = 0 follows 1: the groups are non-decreasing and none is empty'),
            (dict(G=4), 'join: group[5] = 2: the last group is G - 1 = 3'),
            (dict(pieces=edit(0, 3, -7)), 'join: gap[0] = -7 overlaps more than min(f[0], f[1]) = 6 samples'),
            (dict(N_out=20), 'join: N_out = 20 is below n_out[0] = 21'),
            (dict(N_out=0), 'join: N_out = 0 is below n_out[0] = 21'),
            (dict(wav=p + 2), 'join: the buffers must be 4-byte aligned'),
            (dict(out=p + 1), 'join: the buffers must be 4-byte aligned')):
        assert join(**kw) == INV and why() == text, (kw, why())
    q, g, pq, pg = _list(*GOOD)
    n_out = (ctypes.c_int64 * 3)()
    assert lib.tts_join_plan(pq, 6, pg, 3, 5, 2003, 7, None) == INV and why() == 'join_plan: a NULL pointer (pieces, group and n_out are required)'
    assert lib.tts_join_plan(pq, 6, pg, 3, 5, 13, 7, n_out) == INV and why() == 'join_plan: count[0] = 13 is not in 1 .. N - first = 2'
    # the speech interval: tts_speech_frames' refusals
    f = ctypes.c_float
    assert lib.tts_speech_interval(None, p, 3, 37, 9, 9, f(0.5), p, p) == INV
    for args, text in (
            ((None, 3, 37, 9, 9, f(0.5), p, p), 'speech_interval: spec, first_active and last_active must not be NULL'),
            ((p, 3, 37, 9, 9, f(0.5), None, p), 'speech_interval: spec, first_active and last_active must not be NULL'),
            ((p, 3, 37, 9, 9, f(0.5), p, None), 'speech_interval: spec, first_active and last_active must not be NULL'),
            ((p, 0, 37, 9, 9, f(0.5), p, p), 'speech_interval: need B, T, F >= 1'),
            ((p, 3, 0, 9, 9, f(0.5), p, p), 'speech_interval: need B, T, F >= 1'),
            ((p, 3, 37, 0, 9, f(0.5), p, p), 'speech_interval: need B, T, F >= 1'),
            ((p, 3, 37, 9, 8, f(0.5), p, p), 'speech_interval: row_stride < F'),
            ((p, 3, 37, 9, 9, f(float('nan')), p, p), 'speech_interval: the threshold is NaN')):
        assert lib.tts_speech_interval(None, *args) == INV and why() == text, (args, why())


def test_the_python_surface_refuses_before_it_touches_a_handle():
    eng = no_device_engine()
    X = np.zeros((5, 2003), np.float32)
    P, Gr = GOOD
    edit = lambda i, j, v: [tuple(v if (a, b) == (i, j) else x for b, x in enumerate(q)) for a, q in enumerate(P)]
    for call, text in (
            (lambda: eng.join(np.zeros(7, np.float32), P, Gr), 'join: a batch (B, N) is needed, got shape (7,)'),
            (lambda: eng.join(X, [], None), "join: pieces must be (P, 4) integers (row, first, count, gap) with P >= 1, got ((0,), dtype('float64'))"),
            (lambda: eng.join(X, [(0, 0, 1)], None), "join: pieces must be (P, 4) integers (row, first, count, gap) with P >= 1, got ((1, 3), dtype('int64'))"),
            (lambda: eng.join(X, [(0, 0, 1.5, 0)], None),
             "join: pieces must be (P, 4) integers (row, first, count, gap) with P >= 1, got ((1, 4), dtype('float64'))"),
            (lambda: eng.join(X, P, [0, 0, 1]), 'join: groups must be 6 integers, got shape (3,) of int64'),
            (lambda: eng.join(X, P, Gr, fade=-1), 'join: fade must be an integer >= 0, got -1'),
            (lambda: eng.join(X, P, Gr, fade=2.5), 'join: fade must be an integer >= 0, got 2.5'),
            (lambda: eng.join(X, P, Gr, fade=(1 << 20) + 1), 'join: fade = 1048577 is larger than tts_join_max_fade() = 1048576'),
            (lambda: eng.join(X, [(0, 0, 1, 0)] * 4097), 'join: 4097 pieces are more than tts_join_max_pieces() = 4096'),
            (lambda: eng.join(X, edit(2, 0, 5), Gr, 7), 'join: row[2] = 5 is not in 0 .. B - 1 = 4'),
            (lambda: eng.join(X, edit(1, 1, 2003), Gr, 7), 'join: first[1] = 2003 is not in 0 .. N - 1 = 2002'),
            (lambda: eng.join(X, edit(3, 2, 1993), Gr, 7), 'join: count[3] = 1993 is not in 1 .. N - first = 1992'),
            (lambda: eng.join(X, P, [1, 1, 1, 2, 2, 2], 7), 'join: group[0] = 1: the groups start at 0'),
            (lambda: eng.join(X, P, [0, 0, 2, 2, 2, 2], 7), 'join: group[2] = 2 follows 0: the groups are non-decreasing and none is empty'),
            (lambda: eng.join(X, edit(0, 3, -7), Gr, 7), 'join: gap[0] = -7 overlaps more than min(f[0], f[1]) = 6 samples'),
            (lambda: eng.join(X, edit(0, 3, -1), Gr, 0), 'join: gap[0] = -1 overlaps more than min(f[0], f[1]) = 0 samples'),
            (lambda: eng.join(X, P, Gr, 7, N_out=20), 'join: N_out = 20 is not in n_out.max() = 21 .. 2^31 - 1'),
            (lambda: eng.join(X, edit(0, 3, 2 ** 31 - 1), Gr, 7), 'join: N_out = 2147483676 is not in n_out.max() = 2147483674 .. 2^31 - 1'),
            (lambda: eng.join(X, [(0, 0, 1, 0)] * 5, [0, 1, 2, 3, 4], 0, N_out=2 ** 31 - 1),
             'join: G * N_out = 10737418235 output samples are more than 2^33 = 8589934592'),
            (lambda: eng.join_plan((5,), P, Gr, 7), 'join_plan: the shape of a batch (B, N) is needed, got (5,)'),
            (lambda: eng.join_plan((5, 13), P, Gr, 7), 'join: count[0] = 13 is not in 1 .. N - first = 2'),
            (lambda: eng.join_plan((0, 13), P, Gr, 7), 'join: need B, N >= 1, got 0, 13'),
            (lambda: eng.speech_interval(np.zeros((3, 37), np.float32), 0.5), 'speech_interval: spec must be a non-empty (B, T, F), got shape (3, 37)'),
            (lambda: eng.speech_interval(np.zeros((3, 37, 9), np.float32), float('nan')), 'speech_interval: the threshold is NaN'),
            (lambda: eng.speech_interval(np.zeros((3, 37, 9), np.float32), 0.5, row_stride=8), 'speech_interval: row_stride 8 < F = 9'),
            (lambda: eng.download_rows(types.SimpleNamespace(shape=(2, 8)), [3]), 'download_rows: 2 lengths in 0 .. 8 are needed, got [3]')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


# ---------------------------------------------------------------------------------------------- the oracle
def test_the_oracles_arithmetic():
    # the fade is symmetric and a cross-fade of two constant signals is constant up to rounding
    for f in (1, 7, 64):
        up = [O.gain(i, 2 * f + 5, f) for i in range(f)]
        down = [O.gain(2 * f + 5 - 1 - i, 2 * f + 5, f) for i in range(f)]
        assert up == down and all(0.0 < a < b for a, b in zip(up[:-1], up[1:])) and up[-1] < 1.0
        assert all(abs(a + b - 1.0) <= 2.0 ** -52 for a, b in zip(up, up[::-1]))
        assert O.gain(f, 2 * f + 5, f) == 1.0 and O.gain(f + 4, 2 * f + 5, f) == 1.0
    assert O.gain(0, 2, 1) == O.gain(1, 2, 1) == 0.5 and O.gain(0, 1, 0) == 1.0
    x = np.arange(1, 41, dtype=np.float32).reshape(2, 20)
    out, n_out = O.join(x, [(0, 2, 6, -2), (1, 0, 5, 3), (0, 19, 1, 0)], [0, 0, 0], 2, 17)
    assert n_out == [13]
    w = [float(O.gain(i, 6, 2)) for i in range(2)]                        # 0.15625, 0.84375
    assert w == [0.15625, 0.84375]
    want = [3 * w[0], 4 * w[1], 5, 6, 7 * w[1] + 21 * w[0], 8 * w[0] + 22 * w[1], 23, 24 * w[1], 25 * w[0], 0, 0, 0, 20, 0, 0, 0, 0]
    assert out[0].tolist() == [float(np.float32(v)) for v in want]
    # -0.0 and NaN: a copied sample keeps its bits, a faded -0.0 stays -0.0, a NaN stays where it contributes
    y = np.array([[-0.0, -0.0, np.nan, 1.0, -0.0, 2.0]], np.float32)
    out, _ = O.join(y, [(0, 0, 6, 0)], [0], 1, 8)
    assert out.view(np.uint32)[0].tolist() == [0x80000000, 0x80000000, 0x7fc00000, 0x3f800000, 0x80000000, 0x3f800000, 0, 0]
    # the interval: both ends of what the end-of-speech oracle finds
    spec = np.zeros((4, 6))
    assert [a.tolist() for a in O.speech_interval_batch(spec.T[None], 0.5)] == [[-1], [-1]]
    spec[2, 1] = spec[0, 4] = 1.0
    spec[1, 5] = np.nan
    assert [a.tolist() for a in O.speech_interval_batch(np.stack([spec.T, np.zeros((6, 4))]), 0.5)] == [[1, -1], [4, -1]]
    # ... and the library and the binding give the oracle's integers
    H = pkg('_hip')
    pieces, groups = [(0, 2, 6, -2), (1, 0, 5, 3), (0, 19, 1, 0)], [0, 0, 0]
    q, g, pq, pg = _list(pieces, groups)
    n = (ctypes.c_int64 * 1)()
    assert H.load_library().tts_join_plan(pq, 3, pg, 1, 2, 20, 2, n) == H.TTS_OK and [n[0]] == n_out == H.join_list(pieces, groups, 2, 20, 2)[3].tolist()
    assert H.join_fades([6, 5, 1], 2).tolist() == O.fades([6, 5, 1], 2)


# ---------------------------------------------------------------------------------------------- split_text
LJ_ABBREVIATIONS = None


def _abbr():
    T = pkg('datasets.text_split')
    ds = pkg('datasets.lj_speech').LJSpeechDatasetHelper(dataset_folder='.', char_dict={'pad': 0, 'eos': 1}, fill_dict=False)
    return T.abbreviations_of(ds)


def _rejoin(pieces):
    out = ''
    for piece, brk in pieces:
        out += piece + ('' if brk == 'cut' else ' ')
    return out.strip()


def test_split_text_on_a_fixed_table():
    T = pkg('datasets.text_split')
    ab = _abbr()
    assert 'mr.' in ab and 'dr.' in ab and all(a.endswith('.') and a == a.lower() for a in ab)
    table = [
        ('', []),
        ('  \n \n ', []),
        ('Hello.', [('Hello.', 'paragraph')]),
        ('One. Two!  Three?', [('One.', 'sentence'), ('Two!', 'sentence'), ('Three?', 'paragraph')]),
        ('Mr. Smith met Dr. Jones. They talked.', [('Mr. Smith met Dr. Jones.', 'sentence'), ('They talked.', 'paragraph')]),
        ('MR. Smith and J. S. Bach paid 3.14 dollars. Really?! "Yes." (He did.) No', [
            ('MR. Smith and J. S. Bach paid 3.14 dollars.', 'sentence'), ('Really?!', 'sentence'), ('"Yes."', 'sentence'), ('(He did.)', 'sentence'),
            ('No', 'paragraph')]),
        ('First paragraph.\nStill the first.\n\nSecond.\n \t\n\n\nThird', [
            ('First paragraph.', 'sentence'), ('Still the first.', 'paragraph'), ('Second.', 'paragraph'), ('Third', 'paragraph')]),
        ('Wait... what', [('Wait...', 'sentence'), ('what', 'paragraph')]),
        ('A version 2.0.1 thing.', [('A version 2.0.1 thing.', 'paragraph')]),
    ]
    for text, want in table:
        assert T.split_text(text, 150, ab) == want, text
    # without the abbreviations 'Mr.' ends a sentence
    assert T.split_text('Mr. Smith.', 150) == [('Mr.', 'sentence'), ('Smith.', 'paragraph')]
    # an over-long sentence: at the last clause break that fits, then at the last blank, then hard
    s = 'alpha beta, gamma delta; epsilon zeta - eta theta: iota kappa lambda'
    assert T.split_text(s, 30) == [('alpha beta, gamma delta;', 'clause'), ('epsilon zeta - eta theta:', 'clause'), ('iota kappa lambda', 'paragraph')]
    assert T.split_text(s, 20) == [('alpha beta,', 'clause'), ('gamma delta;', 'clause'), ('epsilon zeta -', 'clause'), ('eta theta:', 'clause'),
                                   ('iota kappa lambda', 'paragraph')]
    assert T.split_text('one two three four five', 9) == [('one two', 'word'), ('three', 'word'), ('four five', 'paragraph')]
    assert T.split_text('1,000 apples, please', 8) == [('1,000', 'word'), ('apples,', 'clause'), ('please', 'paragraph')]
    word = 'x' * 400
    assert T.split_text(word, 150) == [('x' * 150, 'cut'), ('x' * 150, 'cut'), ('x' * 100, 'paragraph')]
    assert T.split_text('ab ' + word + '. End.', 150)[:2] == [('ab', 'word'), ('x' * 150, 'cut')]
    assert T.MAX_CHARS == 150 and inspect.signature(T.split_text).parameters['max_chars'].default == 150
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            T.split_text('a', bad)
    with pytest.raises(ValueError):
        T.split_text(b'a')


def test_split_text_properties():
    T = pkg('datasets.text_split')
    ab = _abbr()
    rng = np.random.RandomState(5)
    words = ['a', 'I', 'the', 'Mr.', 'dr.', 'J.', '3.14', 'cat,', 'sat;', 'on:', '-', 'mat.', 'Why?', 'No!', '"so."', '(well.)', 'x' * 37, 'y' * 170,
             'end...', '1,000']
    blanks = [' ', ' ', ' ', '  ', '\t', '\n', '\n\n', ' \n \n', '\n\n\n']
    for trial in range(200):
        n = int(rng.randint(1, 60))
        text = ''.join(words[rng.randint(len(words))] + blanks[rng.randint(len(blanks))] for _ in range(n))
        for max_chars in (1, 7, 40, 150):
            got = T.split_text(text, max_chars, ab)
            assert got == T.split_text(text, max_chars, ab)                                  # deterministic
            assert all(1 <= len(p) <= max_chars and b in T.BREAKS for p, b in got)
            assert all(p == p.strip() and '  ' not in p and '\n' not in p for p, _b in got)
            assert _rejoin(got) == ' '.join(text.split())                                    # nothing lost but whitespace
            assert got[-1][1] == 'paragraph'
            paragraphs = [q for q in __import__('re').split(r'\n[^\S\n]*\n', text) if q.strip()]
            assert sum(b == 'paragraph' for _p, b in got) == len(paragraphs)
            if max_chars >= 170:
                assert all(b != 'cut' for _p, b in got)


# ---------------------------------------------------------------------------------------------- inference
def test_the_pause_and_fade_conversions():
    inf = pkg('tacotron.inference')
    assert inf.PAUSES_MS == {'paragraph': 700.0, 'sentence': 350.0, 'clause': 120.0, 'word': 0.0, 'cut': 0.0} and inf.FADE_MS == 5.0
    assert inf.pause_samples(None, 22050) == {'paragraph': 15434, 'sentence': 7717, 'clause': 2646, 'word': 0, 'cut': 0}
    assert inf.pause_samples({'sentence': 100, 'cut': 1.0}, 8000) == {'paragraph': 5600, 'sentence': 800, 'clause': 960, 'word': 0, 'cut': 8}
    assert inf.fade_samples(5.0, 22050) == 110 and inf.fade_samples(0, 22050) == 0 and inf.fade_samples(0.01, 22050) == 0
    for bad in ({'pause': 1.0}, {'sentence': -1.0}, {'sentence': float('nan')}, {'sentence': float('inf')}, {'sentence': 'long'}, [350.0], {'word': 1e12}):
        with pytest.raises(ValueError):
            inf.pause_samples(bad, 22050)
    for bad in (-1.0, float('nan'), float('inf'), 'short', None, 1e6):
        with pytest.raises(ValueError):
            inf.fade_samples(bad, 22050)
    # lead = max(0, floor(max(0, first_active - 1) / rate) - keep_frames)
    assert [inf.lead_frames(fa, 1.0, 0) for fa in (0, 1, 2, 10)] == [0, 0, 1, 9]
    assert inf.lead_frames(10, 1.0, 4) == 5 and inf.lead_frames(10, 1.0, 20) == 0
    assert inf.lead_frames(10, 2.0, 0) == 4 and inf.lead_frames(10, 0.5, 3) == 15 and inf.lead_frames(12, 1.3, 1) == 7


def test_the_edit_list_of_a_call():
    inf = pkg('tacotron.inference')
    pauses = {'paragraph': 700, 'sentence': 350, 'clause': 120, 'word': 0, 'cut': 0}
    texts = [0, 0, 0, 1, 2, 2, 3]
    breaks = ['sentence', 'clause', 'paragraph', 'paragraph', 'sentence', 'paragraph', 'paragraph']
    n_frames = [10, 8, 6, 9, 7, 5, 4]
    first = [3, -1, 1, 0, -1, 2, -1]
    q, g, said, tail, orphans = inf.join_list_of_call(texts, breaks, n_frames, first, 10, pauses, 1.0, 1, True)
    # row 1 is silent: its 120 go behind row 0; row 4 opens text 2 in this call and is silent, and so is all of text 3: their pauses
    # are the caller's to put behind what an earlier call said of those texts
    assert q.tolist() == [[0, 10, 80, 470], [2, 0, 50, 700], [3, 0, 80, 700], [5, 0, 40, 700]]
    assert g.tolist() == [0, 0, 1, 2] and said == [0, 1, 2] and tail == [700, 700, 700] and orphans == [(2, 350), (3, 700)]
    q, _g, _s, _t, _o = inf.join_list_of_call(texts, breaks, n_frames, first, 10, pauses, 1.0, 0, False)
    assert q[:, 1].tolist() == [0, 0, 0, 0] and q[:, 2].tolist() == [90, 50, 80, 40]
    q, g, said, tail, orphans = inf.join_list_of_call([0], ['paragraph'], [3], [-1], 10, pauses, 1.0, 0, True)
    assert q.shape == (0, 4) and said == [] and tail == [] and orphans == [(0, 700)]


class _Dataset(object):
    _abbreviations = {'mr.': 'mister', 'etc': 'etcetera'}

    def process_sentences(self, sentences):
        rows = [np.array([ord(c) for c in s.lower().replace('mr.', 'mister')] + [1], np.int32) for s in sentences]
        return [r.tobytes() for r in rows], [len(r) for r in rows]


def test_the_packing():
    inf = pkg('tacotron.inference')
    texts = ['Mr. A came. He left, and that was all there is to say about it.', '', 'Second text.']
    calls, piece_text, piece_break, pieces = inf.pack_pieces(texts, _Dataset(), 2, 30)
    assert pieces == ['Mr. A came.', 'He left,', 'and that was all there is to', 'say about it.', 'Second text.']
    assert piece_text == [0, 0, 0, 0, 2] and piece_break == ['sentence', 'clause', 'word', 'paragraph', 'paragraph']
    assert [(p0, ids.shape) for p0, ids in calls] == [(0, (2, 15)), (2, (2, 29)), (4, (1, 13))]
    pad = pkg('tacotron.params').dataset_params.vocabulary_dict['pad']
    assert calls[0][1][1].tolist() == [ord(c) for c in 'he left,'] + [1] + [pad] * 6 and calls[0][1].dtype == np.int32
    assert inf.pack_pieces(['', ' \n\n '], _Dataset(), 64, 150) == ([], [], [], [])
    for bad in (0, -1, 2.5, None):
        with pytest.raises(ValueError):
            inf.pack_pieces(texts, _Dataset(), bad, 150)
    with pytest.raises(ValueError):
        inf.pack_pieces('one string', _Dataset(), 64, 150)


def test_synthesize_text_refuses_a_bad_setting_before_it_touches_an_engine():
    inf = pkg('tacotron.inference')
    model = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params)     # no engine: touching it is an AttributeError
    for kw in (dict(momentum=2.0), dict(speaking_rate=9.0), dict(pitch=3.0), dict(phase_init='guess'), dict(loudness=float('nan')),
               dict(loudness=(-23.0, 0.0)), dict(stop_at_silence_db=None), dict(stop_at_silence_db=float('nan')), dict(silence_keep_ms=-1.0),
               dict(pauses_ms={'breath': 1.0}), dict(pauses_ms={'word': -1.0}), dict(fade_ms=-1.0), dict(fade_ms=1e9), dict(batch_size=0),
               dict(max_chars=0)):
        with pytest.raises(ValueError):
            inf.synthesize_text(model, ['A text.'], _Dataset(), **kw)
    with pytest.raises(ValueError):
        inf.synthesize_texts(['A text.'], None, out_dir=ROOT, momentum=2.0)
    with pytest.raises(ValueError):
        inf.synthesize_texts(['A text.'], None, out_dir=ROOT, pauses_ms={'breath': 1.0})
    sig = inspect.signature(inf.synthesize_text).parameters
    assert (sig['batch_size'].default, sig['pauses_ms'].default, sig['fade_ms'].default, sig['lead_trim'].default) == (64, None, 5.0, True)


def test_the_command_line_parses(tmp_path):
    inf = pkg('tacotron.inference')
    args = inf.parse_args([])
    assert (args.text, args.max_chars, args.pause_ms, args.fade_ms) == (False, 150, [], 5.0)
    # ... and every option that was there reads what it read
    assert (args.synthesis_file, args.synthesis_dir, args.weights, args.synthetic_weights, args.device, args.seed) == (None, None, None, None, 0, 0)
    assert (args.momentum, args.stop_at_silence, args.silence_keep_ms, args.rate, args.pitch, args.phase_init) == (0.0, None, 100.0, 1.0, 0.0, 'random')
    assert (args.loudness, args.max_peak, args.check_alignment) == (None, 1.0, False)
    args = inf.parse_args(['--text', '--max-chars', '80', '--pause-ms', 'sentence=200', '--pause-ms', 'clause=50.5', '--fade-ms', '2'])
    assert (args.text, args.max_chars, dict(args.pause_ms), args.fade_ms) == (True, 80, {'sentence': 200.0, 'clause': 50.5}, 2.0)
    for bad in (['--pause-ms', 'breath=1'], ['--pause-ms', 'sentence'], ['--pause-ms', 'sentence=long'], ['--max-chars', 'many']):
        with pytest.raises(SystemExit):
            inf.parse_args(bad)
    path = tmp_path / 'texts.txt'
    path.write_text('One line. Two sentences.\nA paragraph.\\n\\nAnother.\n')
    assert inf.read_texts(str(path)) == ['One line. Two sentences.', 'A paragraph.\n\nAnother.']
