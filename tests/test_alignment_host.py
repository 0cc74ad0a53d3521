"""Attention diagnostics without a GPU: the numpy oracle of tests/alignment_oracle.py on hand-written utterances whose records are
written out literally and on the alignment the reference dumped; ``tacotron.attention_check.verdict`` on cases far from any
sensible threshold; the symbols, the 56-byte record, every refusal of the library (on a NULL handle) and of the Python surface (on
an engine that never had a handle); the command lines."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import alignment_cases as C
import alignment_oracle as O
from conftest import ROOT, pkg
from host_checks import no_device_engine


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('name', list(C.HAND))
def test_the_oracle_on_hand_written_cases(name):
    rows, N, want, durations, pos = C.HAND[name]
    rec, dur, p, peak = O.utterance(rows, N)
    for field, value in want.items():
        assert (np.isnan(rec[field]) and np.isnan(value)) if isinstance(value, float) and np.isnan(value) else rec[field] == value, \
            (name, field, rec[field], value)
    assert list(dur) == durations and list(p) == pos
    assert np.array_equal(peak.view(np.uint32), rows[np.arange(len(pos)), pos].view(np.uint32))


def test_the_hand_written_cases_cover_what_they_are_named_for():
    rec = {name: C.HAND[name][2] for name in C.HAND}
    assert rec['tie']['end_step'] == -1 and C.HAND['tie'][4][0] == 0                     # .5 .5: the lower index
    assert np.isnan(rec['first_nan']['focus_sum']) and C.HAND['first_nan'][4][1] == 1    # the first of two NaNs
    assert rec['end_at_0']['end_step'] == 0 and rec['end_at_0']['after_end'] == 2
    assert rec['no_end']['end_step'] == -1 and rec['no_end']['after_end'] == 0
    assert rec['backward']['backward'] == 1 and rec['backward']['max_back'] == 2
    assert rec['stall']['longest_stall'] == 3
    assert rec['off_text']['off_text'] == 2
    assert rec['first_nan']['skipped'] == 1


def test_the_oracle_in_a_ragged_batch_is_the_oracle_alone():
    ali, n_sent, n_steps, names = C.hand_batch()
    records, durations, pos, peak = O.batch(ali, n_sent, n_steps)
    for b, name in enumerate(names):
        rows, N, want, dur, p = C.HAND[name]
        alone = O.utterance(rows, N)[0]
        for field in O.FIELDS:
            assert records[field][b] == alone[field] == want[field], (name, field)
        assert list(durations[b, :rows.shape[1]]) == dur and not durations[b, rows.shape[1]:].any()
        assert list(pos[b, :len(p)]) == p and np.all(pos[b, len(p):] == -1) and not peak[b, len(p):].any()
    assert O.same_records(records, records.copy()) and not O.same_records(records, records[::-1])


def test_the_oracle_on_the_reference_fixture():
    rows = C.fixture()
    assert rows.shape == (200, 92) and 0.0107 < rows.min() and rows.max() < 0.0110      # flat
    rec = O.utterance(rows, 92)[0]
    assert rec['end_step'] == 0 and rec['after_end'] == 142 and round(rec['focus_sum'] / 200, 4) == 0.0109
    rec60 = O.utterance(rows, 60)[0]
    assert rec60['end_step'] == -1 and rec60['off_text'] == 70 and rec60['longest_stall'] == 96


def test_text_lengths_oracle():
    ids = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [3, 0, 4, 0], [1, 2, 3, 4]], np.int32)
    assert list(O.text_lengths(ids)) == [1, 1, 3, 4]
    assert list(O.text_lengths(ids, pad_id=4)) == [4, 4, 4, 3]          # (0 is a character then)


# ---------------------------------------------------------------------------------------------- the verdict
def test_the_verdict_marks_the_fixture_unfocused():
    A = pkg('tacotron.attention_check')
    rows = C.fixture()
    rec = O.utterance(rows, 92)[0]
    assert abs(A.mean_focus(rec) - 1.0 / 92) < 2e-4                        # a flat alignment: 1 / N, fifteen times under the default
    v = A.verdict(rec)
    assert 'unfocused' in v and 'wander' in v and 'unfinished' not in v
    v60 = A.verdict(O.utterance(rows, 60)[0])
    assert {'unfinished', 'unfocused', 'off_text', 'stall', 'backward'} <= set(v60)
    assert set(v60) <= set(A.FLAGS) and list(v60) == [f for f in A.FLAGS if f in v60]      # the order of FLAGS
    line = A.summary(rec)
    assert line.startswith('unfocused wander: 92 tokens in 200 steps') and '\n' not in line


def test_the_verdict_is_empty_for_a_clean_monotone_alignment():
    A = pkg('tacotron.attention_check')
    rows, N = C.monotone()
    rec = O.utterance(rows, N)[0]
    assert 0.6 < A.mean_focus(rec) < 0.8 and rec['max_jump'] == 1 and rec['longest_stall'] == 2
    assert rec['end_step'] == 29 and rec['after_end'] == 0 and rec['skipped'] == 0 and rec['backward'] == 0 and rec['off_text'] == 0
    assert A.verdict(rec) == ()
    assert A.summary(rec).startswith('clean: 17 tokens in 40 steps')
    # a batch of records in, a list of tuples out; thresholds are the caller's
    records = O.batch(np.ascontiguousarray(rows[:, None, :]), [N])[0]
    assert A.verdict(records) == [()]
    assert A.verdict(records, min_focus=0.9) == [('unfocused',)]
    assert A.verdict(records, max_jump=0, max_stall_steps=1) == [('skip', 'stall')]
    rep = A.report(records)
    assert rep[0]['index'] == 0 and rep[0]['verdict'] == [] and rep[0]['record']['n_sent'] == 17
    import json
    assert json.loads(json.dumps(rep))[0]['record']['end_step'] == 29
    with pytest.raises(ValueError):
        A.verdict(np.zeros(3))
    assert 'untuned' in A.__doc__.lower() and 'untuned' in A.verdict.__doc__.lower()


def test_every_hand_case_gets_the_flags_of_its_record():
    A = pkg('tacotron.attention_check')
    records = O.batch(*C.hand_batch()[:3])[0]
    got = dict(zip(C.hand_batch()[3], A.verdict(records)))
    assert got['clean'] == () and got['stall'] == () and got['backward'] == ()          # (a stall of 3 and a step back of 2: under the defaults)
    assert got['tie'] == ('unfinished',) and got['no_end'] == ('unfinished',)
    assert got['first_nan'] == ('unfocused',) and got['off_text'] == ('off_text',)


# ---------------------------------------------------------------------------------------------- the library, without a device
NAMES = ('tts_alignment_stats', 'tts_text_lengths', 'tts_set_alignment_stats', 'tts_synth_alignment_stats', 'tts_wait_host_alignment_stats')


def test_symbols_and_the_record():
    H = pkg('_hip')
    lib = H.load_library()
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert ctypes.sizeof(H.TtsAlignmentStats) == 56 and H.ALIGNMENT_RECORD.itemsize == 56
    assert H.ALIGNMENT_RECORD == O.RECORD
    assert [n for n, _t in H.TtsAlignmentStats._fields_] == list(O.FIELDS) + ['focus_sum']
    assert H.TtsAlignmentStats.focus_sum.offset == 48
    assert '"alignment"' in header and 'tts_alignment_stats_t' in header


def _i32(values):
    arr = (ctypes.c_int32 * len(values))(*values)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal is made on the arguments alone, ahead of the handle: with a NULL handle a bad call and a good one are both
    refused, but only the bad one with its own reason.  The pointers are never dereferenced."""
    H = pkg('_hip')
    lib = H.load_library()
    INV = H.TTS_ERR_INVALID
    p = 4096   # any aligned non-NULL address

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    assert lib.tts_alignment_stats(None, p, 200, 3, 92, _i32([92, 1, 60]), _i32([200, 1, 17]), p, p, p, p) == INV   # only the handle is missing
    for args, text in (
            ((None, 200, 3, 92, None, None, p, None, None, None), 'alignment_stats: a NULL pointer (alignments and stats are required)'),
            ((p, 200, 3, 92, None, None, None, None, None, None), 'alignment_stats: a NULL pointer (alignments and stats are required)'),
            ((p, 200, 0, 92, None, None, p, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
            ((p, 200, 3, 0, None, None, p, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
            ((p, 0, 3, 92, None, None, p, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
            ((p, 200, 3, 92, _i32([92, 0, 60]), None, p, None, None, None), 'alignment_stats: n_sent[1] = 0 is not in 1 .. Ts = 92'),
            ((p, 200, 3, 92, _i32([92, 1, 93]), None, p, None, None, None), 'alignment_stats: n_sent[2] = 93 is not in 1 .. Ts = 92'),
            ((p, 200, 3, 92, None, _i32([201, 1, 1]), p, None, None, None), 'alignment_stats: n_steps[0] = 201 is not in 1 .. n_steps_max = 200'),
            ((p, 200, 3, 92, None, _i32([200, 1, -5]), p, None, None, None), 'alignment_stats: n_steps[2] = -5 is not in 1 .. n_steps_max = 200'),
            ((p, 200, 3, 92, None, None, p + 4, None, None, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p + 1, 200, 3, 92, None, None, p, None, None, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p, 200, 3, 92, None, None, p, p + 2, None, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p, 200, 3, 92, None, None, p, None, p + 2, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
            ((p, 200, 3, 92, None, None, p, None, None, p + 2), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned')):
        assert lib.tts_alignment_stats(None, *args) == INV and why() == text, (args, why())
    assert lib.tts_text_lengths(None, p, 3, 92, 0, p) == INV
    for args, text in (((None, 3, 92, 0, p), 'text_lengths: a NULL pointer (ids and n_sent are required)'),
                       ((p, 3, 92, 0, None), 'text_lengths: a NULL pointer (ids and n_sent are required)'),
                       ((p, 0, 92, 0, p), 'text_lengths: need B, Ts >= 1'),
                       ((p, 3, 0, 0, p), 'text_lengths: need B, Ts >= 1'),
                       ((p + 2, 3, 92, 0, p), 'text_lengths: the buffers must be 4-byte aligned')):
        assert lib.tts_text_lengths(None, *args) == INV and why() == text, (args, why())
    assert lib.tts_set_alignment_stats(None, 1, 0) == INV
    assert lib.tts_synth_alignment_stats(None, p, 3) == INV
    assert lib.tts_wait_host_alignment_stats(None, 0, None, None) == INV


# ---------------------------------------------------------------------------------------------- the Python surface
def test_the_python_surface_refuses_before_it_touches_a_handle():
    H = pkg('_hip')
    eng = no_device_engine()
    X = np.zeros((200, 3, 92), np.float32)
    ids = np.zeros((3, 92), np.int32)
    for call, text in (
            (lambda: eng.alignment_stats(np.zeros((200, 92), np.float32)), 'alignment_stats: alignments (n_steps_max, B, Ts) are needed, got shape (200, 92)'),
            (lambda: eng.alignment_stats(np.zeros((200, 0, 92), np.float32)), 'alignment_stats: alignments (n_steps_max, B, Ts) are needed, got shape (200, 0, 92)'),
            (lambda: eng.alignment_stats(X, n_sent=[92, 0, 60]), 'n_sent[1] = 0 is not in 1 .. Ts = 92'),
            (lambda: eng.alignment_stats(X, n_sent=[92, 1, 93]), 'n_sent[2] = 93 is not in 1 .. Ts = 92'),
            (lambda: eng.alignment_stats(X, n_sent=[92, 1]), 'n_sent: 3 integers are needed, got shape (2,) of int64'),
            (lambda: eng.alignment_stats(X, n_sent=[92.0, 1.0, 60.0]), 'n_sent: 3 integers are needed, got shape (3,) of float64'),
            (lambda: eng.alignment_stats(X, n_steps=[201, 1, 1]), 'n_steps[0] = 201 is not in 1 .. n_steps_max = 200'),
            (lambda: eng.alignment_stats(X, n_steps=[200, 1, -1]), 'n_steps[2] = -1 is not in 1 .. n_steps_max = 200'),
            (lambda: eng.alignment_stats(X, n_steps=np.ones((3, 1), np.int32)), 'n_steps: 3 integers are needed, got shape (3, 1) of int32'),
            (lambda: eng.text_lengths(np.zeros(92, np.int32)), 'text_lengths: ids (B, Ts) are needed, got shape (92,)'),
            (lambda: eng.text_lengths(ids, pad_id=0.5), 'text_lengths: pad_id must be an int32, got 0.5'),
            (lambda: eng.text_lengths(ids, pad_id=2 ** 31), 'text_lengths: pad_id must be an int32, got 2147483648'),
            (lambda: eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, alignment_stats='yes'),
             "alignment_stats must be None, a bool or (enabled, pad_id), got 'yes'"),
            (lambda: eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, alignment_stats=0),
             'alignment_stats must be None, a bool or (enabled, pad_id), got 0'),
            (lambda: eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, alignment_stats=(True, 0.5)),
             'alignment_stats must be None, a bool or (enabled, pad_id), got (True, 0.5)'),
            (lambda: eng.set_alignment_stats(True, pad_id=2 ** 31), 'alignment_stats must be None, a bool or (enabled, pad_id), got (True, 2147483648)')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    S = H.alignment_stats_setting
    assert S(None) is None and S(False) == (False, 0) and S(True) == (True, 0) and S((True, 7)) == (True, 7) and S((False, 3)) == (False, 3)
    assert eng._alignment_stats == (False, 0)


def test_the_keyword_is_threaded_through_the_entry_points():
    inf, serve, ev = pkg('tacotron.inference'), pkg('tacotron.serve'), pkg('tacotron.evaluate')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host):
        assert inspect.signature(fn).parameters['alignment_stats'].default is None, fn
    for fn in (inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences, serve.serve):
        assert inspect.signature(fn).parameters['check_alignment'].default is False, fn
    for fn in (ev.evaluate, ev.evaluate_checkpoint):
        assert inspect.signature(fn).parameters['attention'].default is False, fn
    assert inf.pad_id() == 0 and inf.REPORT_FILE == 'alignment_report.json'
    assert inspect.signature(pkg('tacotron.gta').write_gta).parameters['attention_stats'].default is False
    assert 'attention_stats' in pkg('tacotron.gta').__doc__


def test_the_command_lines_parse(capsys):
    inf = pkg('tacotron.inference')
    assert inf.parse_args([]).check_alignment is False
    assert inf.parse_args(['--check-alignment']).check_alignment is True
    with pytest.raises(SystemExit) as e:
        inf.parse_args(['--help'])
    assert e.value.code == 0 and '--check-alignment' in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        pkg('tacotron.evaluate').main(['--help'])
    assert e.value.code == 0 and '--attention' in capsys.readouterr().out
