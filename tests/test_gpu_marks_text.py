"""GPU: the time map of the timing marks end to end, on the synthetic network of tests/test_gpu_long_text.py.  ``synthesize_text``
on a two-sentence text with ``marks``: the waveforms keep their bits, every mark lies inside what is delivered, the marks are
ordered across the join, and the sentence marks begin where the join lays their pieces -- o[p], computed by hand from the edit
list and tts_join_plan -- in one call and with the text cut over two calls; then the same through an output rate of 8 kHz."""
import numpy as np
import pytest

import eos_cases as E
import marks_oracle as MO
from test_gpu_long_text import FADE_MS, MAX_CHARS, N_ITER, PAUSES, SEED, Case, bits

pytestmark = pytest.mark.gpu

TEXT = ['The cat sat. It ran far away.']


@pytest.fixture(scope='module')
def case():
    """the long-text case with a stopping threshold of this text's own: below the loudest frame of its quietest piece in either
    packing (a call's spectrograms depend on the length its ids are padded to), so that every piece has an active frame"""
    c = Case()
    tops, values = [], []
    for batch_size in (64, 1):
        for _p0, ids in c.I.pack_pieces(TEXT, c.dataset, batch_size, MAX_CHARS)[0]:
            lin = c.by_hand(ids, SEED, stop=None)['linear'].to_host()
            mx = np.clip(lin.astype(np.float64), 0.0, 1.0).max(axis=2)
            tops.append(mx.max(axis=1).min())
            values.append(mx.ravel())
    top, values = min(tops), np.unique(np.concatenate(values))
    below = values[values < top - 2.2 * E.OFF_THRESHOLD]
    assert len(below), 'no frame lies clearly below the quietest piece\'s loudest one'
    c.threshold_db = float(np.float32(((below[-1] + top) / 2.0 - 1.0) * E.RANGE_DB + E.REF_DB))
    c.settings = dict(c.settings, stop_at_silence_db=c.threshold_db)
    yield c
    c.engine.close()


def run(c, **kw):
    return c.I.synthesize_text(c.model, TEXT, c.dataset, pauses_ms=PAUSES, fade_ms=FADE_MS, max_chars=MAX_CHARS, n_steps=c.S, n_iter=N_ITER,
                               seed=SEED, **dict(c.settings, **kw))


def by_hand(c, batch_size):
    """per piece where the join lays it in the text's waveform -- (offset, first, count) -- from calls made by hand"""
    calls, piece_text, piece_break, pieces = c.I.pack_pieces(TEXT, c.dataset, batch_size, MAX_CHARS)
    assert pieces == ['The cat sat.', 'It ran far away.']
    thr = c.engine.speech_threshold(c.threshold_db, E.REF_DB, E.MAX_DB)
    laid, total, tail = [], 0, 0
    for k, (p0, ids) in enumerate(calls):
        res = c.by_hand(ids, SEED + k)
        first_active = c.engine.speech_interval(res['linear'], thr)[0].to_host()
        B = len(ids)
        rows, groups, said, tails, orphans = c.I.join_list_of_call(piece_text[p0:p0 + B], piece_break[p0:p0 + B], res['n_frames'], first_active,
                                                                   c.hop, c.pauses, 1.0, c.keep, True)
        assert len(rows) == B and not orphans                                   # every piece speaks
        n_out = c.engine.join_plan(res['wav'].shape, rows, groups, c.fade).tolist()
        part = total + tail if laid else 0
        o = 0
        for row in rows:
            laid.append((part + o, int(row[1]), int(row[2])))
            o += int(row[2]) + int(row[3])
        assert o - int(rows[-1][3]) == n_out[0]                                 # the layout rule is tts_join_plan's
        total, tail = part + n_out[0], tails[0]
    return laid, total


@pytest.mark.parametrize('batch_size', [64, 1])
def test_sentence_marks_begin_where_the_join_lays_their_pieces(case, batch_size):
    c = case
    plain = run(c, batch_size=batch_size)
    wavs, marks = run(c, batch_size=batch_size, marks='word', marks_max_jump=3)
    assert len(wavs) == len(marks) == 1 and np.array_equal(bits(wavs[0]), bits(plain[0]))
    laid, total = by_hand(c, batch_size)
    n = len(wavs[0])
    assert n == total and len(laid) == 2
    sentences = [m for m in marks[0] if m['type'] == 'sentence']
    words = [m for m in marks[0] if m['type'] == 'word']
    assert [m['value'] for m in sentences] == ['The cat sat', 'It ran far away']          # (the front end drops the full stops)
    assert [m['value'] for m in words] == ['The', 'cat', 'sat', 'It', 'ran', 'far', 'away']
    for m, (o, _first, count) in zip(sentences, laid):
        assert m['sample'] == o and o <= m['end_sample'] <= o + count and m['spoken'] and isinstance(m['reliable'], bool)
    assert sentences[1]['sample'] > sentences[0]['end_sample']                  # the pause lies between them
    for m in marks[0]:
        assert 0 <= m['sample'] <= m['end_sample'] <= n and m['value'] == TEXT[0][m['start']:m['end']]
        assert abs(m['time_ms'] - 1000.0 * m['sample'] / 22050) < 0.03 and m['time_ms'] <= m['end_ms']   # (half a sample)
    assert all(a['sample'] <= b['sample'] and a['end_sample'] <= b['end_sample'] for a, b in zip(words[:-1], words[1:]))
    # every border is a decoder step of its piece: a multiple of r * hop behind the piece's row start, or an edge of its cut
    step = c.hp.reduction * c.hop
    for m, (o, first, count) in zip(sentences, laid):
        inside = [w for w in words if m['sample'] <= w['sample'] and w['end_sample'] <= m['end_sample']]
        assert inside
        for w in inside:
            for x in (w['sample'], w['end_sample']):
                assert x in (o, o + count) or (x - o + first) % step == 0, (w, o, first, count)
    chars = run(c, batch_size=batch_size, marks='char')[1][0]
    assert [m for m in chars if m['type'] != 'char'] == run(c, batch_size=batch_size, marks='word')[1][0]
    assert ''.join(m['value'] for m in chars if m['type'] == 'char') == TEXT[0].replace(' ', '').replace('.', '')


def test_through_an_output_rate_and_with_the_diagnostics(case):
    c = case
    wavs, records, verdicts, piece_text, marks = run(c, marks='word', check_alignment=True, output=('pcm16', None, 8000))
    assert len(records) == 2 and piece_text == [0, 0] and wavs[0].dtype == np.int16
    full = run(c, marks='word')[1][0]
    n = len(wavs[0])
    for m, f in zip(marks[0], full):
        assert 0 <= m['sample'] <= m['end_sample'] <= n
        assert m['sample'] == min(int(np.floor(f['sample'] * 8000 / 22050 + 0.5)), n) and m['time_ms'] == f['time_ms']
    # the path behind the marks is the oracle's on the call's own alignments
    calls = c.I.pack_pieces(TEXT, c.dataset, 64, MAX_CHARS)[0]
    res = c.engine.synthesize(calls[0][1], c.S, E.REF_DB, E.MAX_DB, E.POWER, N_ITER, c.win, c.hop, seed=SEED, peak_normalize=False, want_alignments=True,
                              stop_at_silence=(c.threshold_db, c.keep), token_times=(True, 0, 4))
    start, stats = c.engine.synth_token_times(2)
    n_sent = c.engine.text_lengths(calls[0][1], 0)
    w_start, w_stats, _p = MO.batch(res['alignments'].to_host(), n_sent, None, 4)
    assert np.array_equal(start, w_start) and MO.same_records(stats, w_stats)
