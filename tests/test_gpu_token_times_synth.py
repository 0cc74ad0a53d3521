"""GPU: the timing marks inside a synthesis call (tts_set_token_times).  With the setting on, start and the records of a call
are, bit for bit, tts_token_times on the alignments the call returned with the sentence lengths taken from its ids on the host --
in the device form and the host form, pipelined and not, with the alignments requested and with them left to the handle's own
buffer, with the alignment statistics beside it and without -- and waveform, mel, alignments, linear and the alignment records
are the bits of the call with the setting off.  With the setting off the call is the call as it was.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, 12 positions of which the third sentence uses 4, 8 decoder steps,
3 Griffin-Lim iterations)."""
import numpy as np
import pytest

import alignment_oracle as AO
import eos_cases as E
import marks_oracle as O
from conftest import pkg
from test_gpu_alignment_synth import SEED, Case, assert_same_outputs, bits

pytestmark = pytest.mark.gpu

J = 2


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def by_hand(case, alignments, ids=None, max_jump=J):
    """the stand-alone call on a call's alignments, the sentence lengths from the ids on the host; held to the oracle too"""
    n_sent = AO.text_lengths(case.ids if ids is None else ids, 0)
    start, stats = case.engine.token_times(alignments, n_sent=n_sent, max_jump=max_jump)
    w_start, w_stats, _path = O.batch(alignments, n_sent, None, max_jump)
    assert np.array_equal(start, w_start) and O.same_records(stats, w_stats)
    return start, stats


def same(got, want):
    return np.array_equal(got[0], want[0]) and O.same_records(got[1], want[1])


@pytest.mark.parametrize('with_stats', [False, True])
@pytest.mark.parametrize('pipeline', [1, 0])
def test_the_results_of_a_call_are_the_stand_alone_call_on_its_alignments(case, pipeline, with_stats):
    eng = case.engine
    want = by_hand(case, case.off['alignments'])
    records = case.by_hand(case.off['alignments'])
    assert list(want[1]['n_sent']) == [12, 12, 4] and np.all(want[1]['n_steps'] == case.S) and np.all(want[0][:, -1] == case.S)
    eng.set_option('pipeline', pipeline)
    try:
        for _ in range(3):                                   # the first call of a setting is not pipelined, the later ones are
            out = case.run(on=with_stats, token_times=(True, 0, J))
            assert same(eng.synth_token_times(case.B), want)
            assert_same_outputs(case.host(out), case.off)    # nothing else of the call changes
            if with_stats:
                assert AO.same_records(eng.synth_alignment_stats(case.B), records)
        for _ in range(3):                                   # alignments == NULL: the handle's own buffer
            out = case.run(on=with_stats, want=False, token_times=(True, 0, J))
            assert same(eng.synth_token_times(case.B), want)
            assert np.array_equal(bits(out['wav'].to_host()), bits(case.off['wav']))
        # another batch and another jump between two: the results are the last call's
        other = E.ids_of(case.case, seed=5)
        out = case.run(on=with_stats, ids=other, token_times=(True, 0, 15))
        assert same(eng.synth_token_times(case.B), by_hand(case, out['alignments'].to_host(), other, 15))
        case.run(on=with_stats, want=False, token_times=(True, 0, J))
        assert same(eng.synth_token_times(case.B), want)
        # a call after the setting was put back is the call as it was
        assert eng._token_times == (False, 0, 4)
        assert_same_outputs(case.host(case.run()), case.off)
        with pytest.raises(pkg('_hip').TtsError) as e:
            eng.synth_token_times(case.B)
        assert 'was not made with tts_set_token_times on' in str(e.value)
    finally:
        eng.set_option('pipeline', 1)


@pytest.mark.parametrize('pipeline', [1, 0])
def test_the_host_form_keeps_the_results_of_three_calls_in_flight(case, pipeline):
    eng = case.engine
    batches = [case.ids, E.ids_of(case.case, seed=5), E.ids_of(case.case, seed=6)]
    batches[2][0, 7:] = 0

    def submit(ids, **kw):
        return eng.synthesize_host(*case.args(ids), seed=SEED, peak_normalize=True, **kw)

    eng.set_option('pipeline', pipeline)
    try:
        off = []
        for t in [submit(ids, want_linear=True, want_alignments=True) for ids in batches]:
            lin, ali = eng.wait_host_outputs(t)
            off.append((eng.wait_host(t), lin, ali))
        for want, with_stats in ((True, False), (False, True)):
            tickets = [submit(ids, want_linear=want, want_alignments=want, alignment_stats=with_stats, token_times=(True, 0, J)) for ids in batches]
            for t, ids, (wav, lin, ali) in zip(tickets, batches, off):
                got = eng.wait_host_token_times(t)
                assert same(got, by_hand(case, ali, ids))                         # ... also from the handle's own buffer
                if with_stats:
                    assert AO.same_records(eng.wait_host_alignment_stats(t), case.by_hand(ali, ids))
                got_lin, got_ali = eng.wait_host_outputs(t)
                if want:
                    assert np.array_equal(bits(got_lin), bits(lin)) and np.array_equal(bits(got_ali), bits(ali))
                assert np.array_equal(bits(eng.wait_host(t)), bits(wav))
            assert same(eng.synth_token_times(case.B), got)                       # the last call's, also in this form
        # a call made with the setting off has nothing to hand out
        t = submit(case.ids)
        with pytest.raises(pkg('_hip').TtsError) as e:
            eng.wait_host_token_times(t)
        assert 'was not made with tts_set_token_times on' in str(e.value)
        assert np.array_equal(bits(eng.wait_host(t)), bits(case.off['wav']))
    finally:
        eng.set_option('pipeline', 1)


def test_the_results_do_not_change_with_the_other_settings(case):
    c, eng = case, case.engine
    want = by_hand(c, c.off['alignments'])
    threshold_db = E.choose_threshold(c.off['linear'], c.case['min_frames'])
    assert threshold_db is not None
    for kw in (dict(stop_at_silence=(threshold_db, 0)), dict(speaking_rate=0.8),
               dict(stop_at_silence=(threshold_db, 0), speaking_rate=0.8, alignment_stats=True)):
        plain = c.engine.synthesize(*c.args(), seed=SEED, want_alignments=True, **kw)
        out = c.engine.synthesize(*c.args(), seed=SEED, want_alignments=True, token_times=(True, 0, J), **kw)
        assert same(eng.synth_token_times(c.B), want), kw
        assert np.array_equal(bits(out['wav'].to_host()), bits(plain['wav'].to_host())), kw
        assert np.array_equal(bits(out['alignments'].to_host()), bits(c.off['alignments'])), kw
        if 'n_frames' in plain:
            assert np.array_equal(out['n_frames'], plain['n_frames'])
    # the host form with a delivery format: the codes are those of the call with the setting off
    kw = dict(stop_at_silence=(threshold_db, 0), speaking_rate=0.8, output=('pcm16', 'none', 22050, 8000))
    t0 = eng.synthesize_host(*c.args(), seed=SEED, **kw)
    codes0, held0, _st = eng.wait_host_encoded(t0)
    t1 = eng.synthesize_host(*c.args(), seed=SEED, token_times=(True, 0, J), **kw)
    assert same(eng.wait_host_token_times(t1), want)
    codes1, held1, _st = eng.wait_host_encoded(t1)
    assert np.array_equal(codes1, codes0) and np.array_equal(held1, held0)


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again: the bits of the handle that never heard of the setting, and no launch in stage
    "alignment" """
    c, eng = case, case.engine
    H = pkg('_hip')
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert_same_outputs(c.host(c.run()), c.off)
        assert eng.profile_get('alignment') == (0.0, 0)
        c.run(token_times=True)
        assert eng.profile_get('alignment')[1] == 3                       # the sentence lengths, the positions and the search
        eng.profile_reset()
        c.run(on=True, token_times=True)
        assert eng.profile_get('alignment')[1] == 4                       # the lengths once, the statistics' two kernels, the search
        eng.profile_reset()
        assert_same_outputs(c.host(c.run()), c.off)
        assert eng.profile_get('alignment') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
    # the handle's setting, read when the call is made; another pad id gives other sentence lengths
    eng.set_token_times(True, pad_id=int(c.ids[1, 0]), max_jump=3)
    try:
        c.run()
        start, stats = eng.synth_token_times(c.B)
        assert list(stats['n_sent']) == list(AO.text_lengths(c.ids, int(c.ids[1, 0]))) and stats['n_sent'][1] == 1
        assert np.all(start[1, 1:] == c.S)
        with pytest.raises(H.TtsError) as e:
            eng.synth_token_times(c.B + 1)
        assert 'the last call had 3 utterances' in str(e.value)
        with pytest.raises(H.TtsError) as e:
            eng._check(eng.lib.tts_set_token_times(eng.handle, 1, 0, 16))
        assert 'set_token_times: max_jump = 16 is not in 1 .. 15' in str(e.value)
    finally:
        eng.set_token_times(False)
    assert eng.lib.tts_set_token_times(None, 0, 0, 4) == H.TTS_ERR_INVALID
    assert_same_outputs(c.host(c.run()), c.off)
