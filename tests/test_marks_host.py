"""CPU: the host side of the timing marks -- which characters make a word and where they came from in the raw text
(tacotron/marks.py: token_spans, piece_spans), where the pieces of a text lie in it (datasets/text_split.py: split_text_spans),
the map from a decoder step to a sample of what is delivered on hand-computed cases (step_sample, marks_of_row, marks_of_text),
the new keyword's refusals through every layer, and which setter calls surround a synthesis call -- with a recording stand-in
for the library (tests/test_settings_host.py).  No GPU."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import marks_oracle as O
from conftest import ROOT, pkg
from test_settings_host import ALL, CALLS, ORDER, SET, KeywordEngine, run
from test_settings_host import eng   # noqa: F401


def helper():
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)


TEXTS = ['Hello there, Mr. Smith [sic].', 'Dr. No. and Mrs. X', 'a.b.', 'plain words only', 'St. Louis, Mo. -- no. five', ' two  blanks ', '']


# ---------------------------------------------------------------------------------------------- text to tokens
@pytest.mark.parametrize('raw', TEXTS)
def test_token_spans_give_the_front_ends_string_and_lie_in_the_raw_text(raw):
    M, ds = pkg('tacotron.marks'), helper()
    processed, spans = M.token_spans(ds, raw)
    ids = np.frombuffer(ds.process_sentences([raw])[0][0], dtype=np.int32)
    assert processed == ds.idx2sent(ids[:-1]) and len(spans) == len(processed)
    assert all(0 <= a < b <= len(raw) for a, b in spans)
    assert all(a1 >= a0 and b1 >= b0 for (a0, b0), (a1, b1) in zip(spans[:-1], spans[1:]))       # ordered
    for c, (a, b) in zip(processed, spans):                   # a character of its own, or one of an abbreviation's expansion
        assert raw[a:b].lower() == c or raw[a:b].lower() in ds._abbreviations


def test_an_expansion_maps_to_its_abbreviation():
    M, ds = pkg('tacotron.marks'), helper()
    processed, spans = M.token_spans(ds, 'Mr. X')
    assert processed == 'mister x' and spans[:6] == [(0, 3)] * 6 and spans[6:] == [(3, 4), (4, 5)]
    assert M.words_of(processed) == [(0, 5), (7, 7)] and M.words_of(' a  bc ') == [(1, 1), (4, 5)] and M.words_of('') == []
    with pytest.raises(ValueError):
        M.token_spans(ds, 'İstanbul')                         # lower case is two characters: no map


def test_split_text_spans_agree_with_split_text():
    T, M, ds = pkg('datasets.text_split'), pkg('tacotron.marks'), helper()
    abbr = T.abbreviations_of(ds)
    texts = ['  Hello   there, Mr. Smith.\tHow are\nyou?\n\n  A second   paragraph; it is long enough to be cut, somewhere, here.  ',
             'One. Two! Three?', 'x' * 40, 'J. S. Bach wrote 3.14 fugues. Then "he stopped." And left.', '', ' \n\n ']
    for text in texts:
        for max_chars in (150, 20, 7):
            got = T.split_text_spans(text, max_chars, abbr)
            assert [(p, k) for p, k, _a, _b in got] == T.split_text(text, max_chars, abbr)
            assert all(' '.join(text[a:b].split()) == p for p, _k, a, b in got)
            assert all(b0 <= a1 for (_p, _k, _a, b0), (_q, _l, a1, _b) in zip(got[:-1], got[1:]))
            for p, _k, a, b in got:
                processed, spans = M.piece_spans(ds, text, a, b)
                assert processed == M.token_spans(ds, p)[0] and all(a <= s < e <= b for s, e in spans)


# ---------------------------------------------------------------------------------------------- steps to samples
R, HOP, SR = 2, 100, 22050
PROCESSED = 'ab cd'
SPANS = [(i, i + 1) for i in range(5)]
START = [0, 1, 2, 3, 5, 6, 8]      # tokens a b _ c d, the end token, and the steps behind it: 8 steps


def row(**kw):
    M = pkg('tacotron.marks')
    kw.setdefault('n_held', 1500)
    return M.marks_of_row(PROCESSED, SPANS, START, R, HOP, rate_in=SR, raw='AB CD', **kw)


def test_step_sample():
    M = pkg('tacotron.marks')
    assert M.step_sample(3, 5, 275, 1.0, 10 ** 6) == 4125.0 and M.step_sample(3, 5, 275, 0.8, 10 ** 6) == 4125.0 / 0.8
    assert M.step_sample(3, 5, 275, 1.25, 10 ** 6) == 3300.0 and M.step_sample(3, 5, 275, 1.0, 4000) == 4000.0
    assert M.step_sample(0, 5, 275, 1.0, 0) == 0.0
    assert M.out_sample(400, 22050, 8000, 10 ** 6) == 145 and M.out_sample(600, 22050, 8000, 10 ** 6) == 218
    assert M.out_sample(600, 22050, 8000, 200) == 200 and M.out_sample(441, 22050, 22050, 10 ** 6) == 441


@pytest.mark.parametrize('rate, scale', [(1.0, 1.0), (0.8, 1.25), (1.25, 0.8)])
def test_the_marks_of_a_row_at_three_rates(rate, scale):
    marks = row(rate=rate, n_held=10 ** 6)
    assert [m['type'] for m in marks] == ['sentence', 'word', 'word'] and [m['value'] for m in marks] == ['AB CD', 'AB', 'CD']
    assert [(m['start'], m['end']) for m in marks] == [(0, 5), (0, 2), (3, 5)]
    want = [(0, 1200), (0, 400), (600, 1200)]                 # the sentence: token 0 to the start of the end token
    for m, (a, b) in zip(marks, want):
        assert (m['sample'], m['end_sample']) == (int(a * scale), int(b * scale)), m
        assert m['time_ms'] == 1000.0 * (a * scale) / SR and m['end_ms'] == 1000.0 * (b * scale) / SR and m['spoken'] is True
    chars = row(rate=rate, n_held=10 ** 6, kind='char')
    assert [m['value'] for m in chars] == ['AB CD', 'AB', 'A', 'B', 'CD', 'C', 'D']
    assert [(m['sample'], m['end_sample']) for m in chars if m['type'] == 'char'] == \
        [(int(a * scale), int(b * scale)) for a, b in ((0, 200), (200, 400), (600, 1000), (1000, 1200))]


def test_an_end_of_speech_cut_in_mid_word_and_another_output_rate():
    marks = row(n_held=1000)
    assert [(m['sample'], m['end_sample']) for m in marks] == [(0, 1000), (0, 400), (600, 1000)]
    marks = row(n_held=1000, rate_out=8000, n_out=363)         # resampled_length(1000, 8000 / 22050) = 363
    assert [(m['sample'], m['end_sample']) for m in marks] == [(0, 363), (0, 145), (218, 363)]
    assert marks[2]['end_ms'] == 1000.0 * 1000 / SR          # the clock does not change with the rate
    marks = row(n_held=1000, rate_out=8000, n_out=300)
    assert marks[2]['end_sample'] == 300                      # never behind what is delivered
    stats = dict(agree=4, n_steps=8)
    assert row(stats=stats)[0]['reliable'] is True and row(stats=dict(agree=3, n_steps=8))[0]['reliable'] is False
    with pytest.raises(ValueError):
        pkg('tacotron.marks').marks_of_row(PROCESSED, SPANS, START[:5], R, HOP, n_held=10)


def test_the_marks_of_a_text_through_trim_join_and_parts():
    """piece 0: a lead trim of 200 samples and 800 kept; piece 1 cross-fades 50 samples into it (a negative gap); piece 2 is
    silent and dropped; piece 3 comes from a second call, whose part starts behind 2000 samples"""
    M = pkg('tacotron.marks')
    pieces = np.array([[0, 200, 800, -50], [1, 0, 500, 300]])
    o = M.join_offsets(pieces, [0, 0])
    assert list(o) == [0, 750] and list(M.join_offsets(np.array([[0, 0, 10, 5], [1, 0, 20, 7], [2, 0, 30, 0]]), [0, 1, 1])) == [0, 0, 27]
    raw = 'AB CD ab cd .. ab cd'
    base = dict(processed=PROCESSED, start=START, stats=None)
    entries = [dict(base, spans=SPANS, n_held=1500, first=200, count=800, o=0, part=0),
               dict(base, spans=[(a + 6, b + 6) for a, b in SPANS], n_held=1500, first=0, count=500, o=750, part=0),
               dict(processed='..', spans=[(12, 13), (13, 14)], start=[0, 0, 0, 8], stats=None, at=1250),
               dict(base, spans=[(a + 15, b + 15) for a, b in SPANS], n_held=1000, first=0, count=1000, o=0, part=2000)]
    marks = M.marks_of_text(entries, R, HOP, rate_in=SR, n_out=3000, raw=raw)
    got = [(m['type'], m['value'], m['sample'], m['end_sample'], m['spoken']) for m in marks]
    assert got == [('sentence', 'AB CD', 0, 800, True), ('word', 'AB', 0, 200, True), ('word', 'CD', 400, 800, True),
                   ('sentence', 'ab cd', 750, 1250, True), ('word', 'ab', 750, 1150, True), ('word', 'cd', 1250, 1250, True),
                   ('sentence', '..', 1250, 1250, False), ('word', '..', 1250, 1250, False),
                   ('sentence', 'ab cd', 2000, 3000, True), ('word', 'ab', 2000, 2400, True), ('word', 'cd', 2600, 3000, True)]
    words = [m for m in marks if m['type'] == 'word']
    assert all(a['sample'] <= b['sample'] for a, b in zip(words[:-1], words[1:]))                # non-decreasing
    assert all(0 <= m['sample'] <= m['end_sample'] <= 3000 and m['value'] == raw[m['start']:m['end']] for m in marks)
    at_8k = M.marks_of_text(entries, R, HOP, rate_in=SR, rate_out=8000, n_out=1088, raw=raw)
    assert [m['end_sample'] for m in at_8k][-1] == 1088 and at_8k[1]['end_sample'] == 73         # floor(200 * 8000 / 22050 + 0.5)


def test_write_marks(tmp_path):
    M = pkg('tacotron.marks')
    path = str(tmp_path / 'm.jsonl')
    M.write_marks(path, row())
    with open(path) as f:
        lines = [json.loads(line) for line in f]
    assert lines == row() and set(lines[0]) == {'type', 'time_ms', 'end_ms', 'sample', 'end_sample', 'start', 'end', 'value', 'spoken'}
    assert 'untuned' in M.__doc__.lower() and 'untuned' in M.reliable.__doc__.lower() and 'not been measured' in M.__doc__
    assert M.reliable(dict(agree=1, n_steps=2)) and not M.reliable(dict(agree=0, n_steps=1)) and O.reliable(dict(agree=1, n_steps=2))


# ---------------------------------------------------------------------------------------------- refusals, before an engine
def test_the_keywords_refusals_through_every_layer(eng):   # noqa: F811
    H, I, S = pkg('_hip'), pkg('tacotron.inference'), pkg('tacotron.serve')
    assert H.token_times_setting(None) is None and H.token_times_setting(True) == (True, 0, 4) and H.token_times_setting(False) == (False, 0, 4)
    assert H.token_times_setting((True, 3, 15)) == (True, 3, 15)
    for bad in (3, 'word', (True, 0), (True, 0, 0), (True, 0, 16), (1, 0, 4), (True, 0.5, 4), (True, 0, True)):
        with pytest.raises(ValueError):
            H.token_times_setting(bad)
        for method in sorted(CALLS):
            with pytest.raises(ValueError):
                run(eng, method, token_times=bad)
    for bad in (0, 16, 2.0, True, None):
        with pytest.raises(ValueError):
            eng.token_times(np.zeros((2, 1, 3), np.float32), max_jump=bad)
    for bad_call in (lambda: eng.token_times(np.zeros((2, 3), np.float32)), lambda: eng.token_times(np.zeros((2, 1, 1025), np.float32)),
                     lambda: eng.token_times(np.zeros((2, 2, 3), np.float32), n_sent=[3, 4]),
                     lambda: eng.token_times(np.zeros((2, 2, 3), np.float32), n_steps=[0, 1]), lambda: eng.set_token_times(True, 0, 16)):
        with pytest.raises(ValueError):
            bad_call()
    assert eng.lib.calls == []
    model = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params, n_steps=lambda: 2, engine=eng)
    ids = np.ones((2, 5), np.int32)
    for kw in (dict(marks='words'), dict(marks=True), dict(marks='word', marks_max_jump=0), dict(marks='char', marks_max_jump=16)):
        for call in (lambda: I.synthesize_batch(model, ids, **kw), lambda: list(I.synthesize_stream(model, [ids], **kw)),
                     lambda: I.synthesize_sentences(['a'], None, **kw), lambda: I.synthesize_text(model, ['a'], helper(), **kw),
                     lambda: I.synthesize_texts(['a'], None, out_dir=ROOT, **kw), lambda: list(S.serve(iter([['a']]), None, **kw))):
            with pytest.raises(ValueError):
                call()
    assert eng.lib.calls == []
    with pytest.raises(SystemExit):
        I.parse_args(['--marks', 'syllable'])
    assert I.parse_args(['--marks']).marks == 'word' and I.parse_args(['--marks', 'char', '--marks-max-jump', '3']).marks_max_jump == 3
    assert I.parse_args([]).marks is None and I.SynthSettings(None).engine_keywords()['token_times'] is None
    assert I.SynthSettings(None, marks='word', marks_max_jump=2).engine_keywords()['token_times'] == (True, 0, 2)


# ---------------------------------------------------------------------------------------------- which setters surround a call
TT = (('tts_set_token_times', (1, 3, 2)), ('tts_set_token_times', (0, 0, 4)))


@pytest.mark.parametrize('method', sorted(CALLS))
def test_off_makes_no_new_call_and_on_is_applied_last_and_put_back_first(eng, method):   # noqa: F811
    H = pkg('_hip')
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[keys.index('token_times')]
    assert (row.mirror, row.initial, row.host_only) == ('_token_times', H.TOKEN_TIMES_OFF, False) and row.check is H.token_times_setting
    assert keys[keys.index('token_times') - 1:keys.index('token_times') + 2] == ['output', 'token_times', 'watermark']
    run(eng, method, **ALL)                                   # the pinned order of tests/test_settings_host.py, unchanged
    assert eng.lib.trace() == [SET[k][0] for k in ORDER] + [CALLS[method]] + [SET[k][1] for k in reversed(ORDER)]
    del eng.lib.calls[:]
    run(eng, method, token_times=None)
    run(eng, method, token_times=False)
    assert eng.lib.trace() == [CALLS[method]] * 2
    del eng.lib.calls[:]
    run(eng, method, token_times=(True, 3, 2), **ALL)
    assert eng.lib.trace() == [SET[k][0] for k in ORDER] + [TT[0], CALLS[method], TT[1]] + [SET[k][1] for k in reversed(ORDER)]
    assert eng._token_times == (False, 0, 4)
    del eng.lib.calls[:]
    if method == 'synthesize_host':                           # ... behind the host form's own setting too
        run(eng, method, token_times=(True, 3, 2), output='pcm16')
        names = [n for n, _a in eng.lib.trace()]
        assert names == ['tts_set_output', 'tts_set_token_times', 'tts_synthesize_host', 'tts_set_token_times', 'tts_set_output']
        del eng.lib.calls[:]
    eng.lib.refuse[CALLS[method][0]] = H.TTS_ERR_INVALID      # a refused call is followed by every put-back
    with pytest.raises(H.TtsError):
        run(eng, method, token_times=True)
    assert eng.lib.trace() == [('tts_set_token_times', (1, 0, 4)), CALLS[method], TT[1]]
    eng.lib.refuse.clear()
    eng.set_token_times(True, 3, 2)                           # the handle's setting as it stands: nothing to set
    del eng.lib.calls[:]
    run(eng, method, token_times=(True, 3, 2))
    assert eng.lib.trace() == [CALLS[method]] and eng._token_times == (True, 3, 2)


# ---------------------------------------------------------------------------------------------- the library, without a device
NAMES = ('tts_token_times', 'tts_token_times_max_tokens', 'tts_set_token_times', 'tts_synth_token_times', 'tts_wait_host_token_times')


def test_symbols_and_the_record():
    H = pkg('_hip')
    lib = H.load_library()
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert ctypes.sizeof(H.TtsTokenTimesStats) == 32 and H.TOKEN_TIMES_RECORD == O.RECORD
    assert [n for n, _t in H.TtsTokenTimesStats._fields_] == ['score'] + list(O.FIELDS)
    assert lib.tts_token_times_max_tokens() == H.TOKEN_TIMES_MAX_TOKENS >= 1024
    INV, p = H.TTS_ERR_INVALID, 4096

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    assert lib.tts_token_times(None, p, 200, 3, 92, None, None, 4, p, p, p) == INV            # only the handle is missing
    for args, code, text in (
            ((None, 200, 3, 92, None, None, 4, p, None, p), INV, 'token_times: a NULL pointer (alignments, start and stats are required)'),
            ((p, 200, 3, 92, None, None, 4, None, None, p), INV, 'token_times: a NULL pointer (alignments, start and stats are required)'),
            ((p, 200, 0, 92, None, None, 4, p, None, p), INV, 'token_times: need B, Ts, n_steps_max >= 1'),
            ((p, 200, 3, 92, None, None, 16, p, None, p), INV, 'token_times: max_jump = 16 is not in 1 .. 15'),
            ((p, 200, 3, 92, None, None, 4, p, p + 2, p), INV, 'token_times: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p, 200, 3, 92, None, None, 4, p, None, p + 4), INV, 'token_times: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p, 200, 3, 1025, None, None, 4, p, None, p), H.TTS_ERR_UNSUPPORTED, 'token_times: Ts = 1025 is above the 1024 tokens of a table')):
        assert lib.tts_token_times(None, *args) == code and why() == text, (args, why())
    assert lib.tts_set_token_times(None, 1, 0, 4) == INV and lib.tts_synth_token_times(None, p, p, 3) == INV
    assert lib.tts_wait_host_token_times(None, 0, None, None, None, None) == INV


def test_the_layers_above_answer_with_marks_last():
    """synthesize_batch and synthesize_stream on an engine that answers with zeros and a staircase of start steps"""
    I = pkg('tacotron.inference')
    H = pkg('_hip')

    class MarkEngine(KeywordEngine):
        def _call(self, ids, keywords):
            self.token_times = keywords['token_times']
            return KeywordEngine._call(self, ids, keywords)

        def synth_token_times(self, B):
            stats = np.zeros(B, H.TOKEN_TIMES_RECORD)
            stats['n_sent'], stats['n_steps'], stats['agree'] = 4, 2, 2
            return np.tile(np.array([0, 1, 1, 2, 2, 2], np.int32), (B, 1)), stats

        def wait_host_token_times(self, ticket):
            return self.synth_token_times(2)

    P = pkg('tacotron.params')
    vocab = P.dataset_params.vocabulary_dict
    ids = np.array([[vocab['a'], vocab[' '], vocab['b'], vocab['eos'], vocab['pad']]] * 2, np.int32)
    for call in (lambda m, **kw: I.synthesize_batch(m, ids, **kw), lambda m, **kw: list(I.synthesize_stream(m, [ids], **kw))[0]):
        model = types.SimpleNamespace(hparams=P.model_params, n_steps=lambda: 2, engine=MarkEngine())
        wavs, marks = call(model, marks='word', marks_max_jump=3)
        assert model.engine.token_times == (True, 0, 3) and len(marks) == 2 and len(wavs) == 2
        r, hop = P.model_params.reduction, 275
        held = hop * (2 * r - 1)                              # the row's samples: step border 2 lies a hop behind them
        assert [(m['type'], m['value'], m['sample'], m['end_sample']) for m in marks[0]] == \
            [('sentence', 'a b', 0, held), ('word', 'a', 0, r * hop), ('word', 'b', r * hop, held)]
        assert marks[0][0]['reliable'] is True
        out = call(model, marks='char', check_alignment=True)
        assert len(out) == 4 and [m['type'] for m in out[-1][1]] == ['sentence', 'word', 'char', 'word', 'char']
        assert not isinstance(call(model), tuple)
