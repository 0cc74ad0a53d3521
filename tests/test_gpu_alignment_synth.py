"""GPU: the attention diagnostics inside a synthesis call (tts_set_alignment_stats).  With the setting on, the records of a call
are, bit for bit, tts_alignment_stats on the alignments the call returned with the sentence lengths taken from its ids on the
host -- in the device form and the host form, pipelined and not, with the alignments requested and with them left to the handle's
own buffer -- and waveform, mel, alignments and linear are the bits of the call with the setting off.  With the setting off the
call is the call as it was.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, 12 positions of which the third sentence uses 4, 8 decoder steps,
3 Griffin-Lim iterations)."""
import copy
import json
import os

import numpy as np
import pytest

import alignment_oracle as O
import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
UP = 4.0 / 12.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(object):
    def __init__(self, case, hp=None, weights=None):
        self.case = case
        self.hp = hp or E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.sampling_rate = 8000          # (the rows are 10 725 samples: blocks to measure at 8 kHz, as test_gpu_loudness_synth.py)
        self.engine.load_weights(weights or E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.S, self.Ts = case['B'], case['S'], case['Ts']
        self.off = self.host(self.run(want=True))            # on a handle whose setting was never touched

    def args(self, ids=None):
        c = self.case
        return (self.ids if ids is None else ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, on=None, want=True, ids=None, **kw):
        return self.engine.synthesize(*self.args(ids), seed=SEED, peak_normalize=True, want_mel=want, want_alignments=want,
                                      want_linear=want, alignment_stats=on, **kw)

    @staticmethod
    def host(out):
        return {k: v.to_host() for k, v in out.items() if k in ('wav', 'mel', 'alignments', 'linear') and v is not None}

    def by_hand(self, alignments, ids=None):
        """the stand-alone call on a call's alignments, the sentence lengths from the ids on the host; held to the oracle too"""
        n_sent = O.text_lengths(self.ids if ids is None else ids, 0)
        records = self.engine.alignment_stats(alignments, n_sent=n_sent)
        assert O.same_records(records, O.batch(alignments, n_sent)[0])
        return records


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def assert_same_outputs(got, want):
    for key in ('wav', 'mel', 'alignments', 'linear'):
        assert np.array_equal(bits(got[key]), bits(want[key])), key


@pytest.mark.parametrize('pipeline', [1, 0])
def test_the_records_of_a_call_are_the_stand_alone_call_on_its_alignments(case, pipeline):
    eng = case.engine
    want = case.by_hand(case.off['alignments'])
    assert list(want['n_sent']) == [12, 12, 4] and np.all(want['n_steps'] == case.S)
    eng.set_option('pipeline', pipeline)
    try:
        for _ in range(3):                                   # the first call of a setting is not pipelined, the later ones are
            out = case.run(on=True)
            records = eng.synth_alignment_stats(case.B)
            assert_same_outputs(case.host(out), case.off)    # nothing else of the call changes
            assert O.same_records(records, want)
        for _ in range(3):                                   # alignments == NULL: the handle's own buffer
            out = case.run(on=True, want=False)
            assert O.same_records(eng.synth_alignment_stats(case.B), want)
            assert np.array_equal(bits(out['wav'].to_host()), bits(case.off['wav']))
        # another batch between two: the records are the last call's
        other = E.ids_of(case.case, seed=5)
        out = case.run(on=True, ids=other)
        assert O.same_records(eng.synth_alignment_stats(case.B), case.by_hand(out['alignments'].to_host(), other))
        case.run(on=True, want=False)
        assert O.same_records(eng.synth_alignment_stats(case.B), want)
    finally:
        eng.set_option('pipeline', 1)
    assert eng._alignment_stats == (False, 0)                # the scope put the handle's setting back


@pytest.mark.parametrize('pipeline', [1, 0])
def test_the_host_form_keeps_the_records_of_three_calls_in_flight(case, pipeline):
    eng = case.engine
    batches = [case.ids, E.ids_of(case.case, seed=5), E.ids_of(case.case, seed=6)]
    batches[2][0, 7:] = 0

    def submit(ids, **kw):
        return eng.synthesize_host(*case.args(ids), seed=SEED, peak_normalize=True, **kw)

    eng.set_option('pipeline', pipeline)
    try:
        # the setting off: what every output has to stay
        off = []
        for t in [submit(ids, want_linear=True, want_alignments=True) for ids in batches]:
            lin, ali = eng.wait_host_outputs(t)
            off.append((eng.wait_host(t), lin, ali))
        assert_same_outputs(dict(wav=off[0][0], linear=off[0][1], alignments=off[0][2], mel=case.off['mel']), case.off)
        for want in (True, False):
            tickets = [submit(ids, want_linear=want, want_alignments=want, alignment_stats=True) for ids in batches]
            for t, ids, (wav, lin, ali) in zip(tickets, batches, off):
                records = eng.wait_host_alignment_stats(t)
                assert O.same_records(records, case.by_hand(ali, ids))            # ... also from the handle's own buffer
                got_lin, got_ali = eng.wait_host_outputs(t)
                if want:
                    assert np.array_equal(bits(got_lin), bits(lin)) and np.array_equal(bits(got_ali), bits(ali))
                else:
                    assert got_lin is None and got_ali is None
                assert np.array_equal(bits(eng.wait_host(t)), bits(wav))
            assert O.same_records(eng.synth_alignment_stats(case.B), records)    # the last call's, also in this form
        # a call made with the setting off has no records to hand out
        t = submit(case.ids)
        with pytest.raises(pkg('_hip').TtsError) as e:
            eng.wait_host_alignment_stats(t)
        assert 'was not made with tts_set_alignment_stats on' in str(e.value)
        assert np.array_equal(bits(eng.wait_host(t)), bits(case.off['wav']))
    finally:
        eng.set_option('pipeline', 1)


def test_stand_alone_calls_between_pipelined_calls_without_a_host_wait(case):
    """tts_synthesize (on), tts_alignment_stats, tts_synthesize (on), ... enqueued through the C ABI on device buffers with no
    synchronisation in between: the stand-alone call runs on the main stream, the statistics of a pipelined call on the front
    stream beside it, and each keeps its own records (they share no scratch)."""
    H = pkg('_hip')
    import alignment_cases as C
    eng, lib, h = case.engine, case.engine.lib, case.engine.handle
    c = case.case
    B, S, Ts = case.B, case.S, case.Ts
    other = E.ids_of(c, seed=5)
    want = {k: case.by_hand(case.run(ids=ids)['alignments'].to_host(), ids) for k, ids in (('a', case.ids), ('b', other))}
    big = C.random_batch(200, 64, 100, tag=7)                       # a stand-alone problem that takes a while
    big_sent = np.array(C.ragged_lengths(64, 100, 8), np.int32)
    big_want = O.batch(big, big_sent)[0]
    d_big, d_ids = eng.to_device(big), {'a': eng.to_device(case.ids), 'b': eng.to_device(other)}
    rounds = 6
    d_alone = [eng.empty((64,), H.ALIGNMENT_RECORD) for _ in range(rounds)]
    d_wav = eng.empty((B, c['hop'] * (S * case.hp.reduction - 1)))
    sp = H.TtsSynthParams(S, E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'], SEED, 1)
    got = []
    eng.set_alignment_stats(True, 0)
    try:
        for k in ('a', 'b'):                                        # (the first call of a setting is not pipelined)
            eng._check(lib.tts_synthesize(h, d_ids[k].data_ptr(), B, Ts, H.byref(sp), None, d_wav.data_ptr(), None, None, None))
        for r in range(rounds):
            k = 'ab'[r % 2]
            eng._check(lib.tts_synthesize(h, d_ids[k].data_ptr(), B, Ts, H.byref(sp), None, d_wav.data_ptr(), None, None, None))
            eng._check(lib.tts_alignment_stats(h, d_big.data_ptr(), 200, 64, 100, H._int32_ptr(big_sent), None, d_alone[r].data_ptr(),
                                               None, None, None))
            k2 = 'ab'[(r + 1) % 2]
            eng._check(lib.tts_synthesize(h, d_ids[k2].data_ptr(), B, Ts, H.byref(sp), None, d_wav.data_ptr(), None, None, None))
            got.append((k2, eng.synth_alignment_stats(B)))           # (waits for that call's decoder alone)
        eng.synchronize()
    finally:
        eng.set_alignment_stats(False)
    for r, (k2, records) in enumerate(got):
        assert O.same_records(records, want[k2]), r
        assert O.same_records(d_alone[r].to_host(), big_want), r
    for a in [d_big, d_wav] + d_alone + list(d_ids.values()):
        a.free()


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
        c.run(on=True)
        assert eng.profile_get('alignment')[1] == 3                       # the sentence lengths and two kernels
        eng.profile_reset()
        assert_same_outputs(c.host(c.run()), c.off)
        assert eng.profile_get('alignment') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
    # the last call was made with the setting off: nothing to fetch
    with pytest.raises(H.TtsError) as e:
        eng.synth_alignment_stats(c.B)
    assert 'was not made with tts_set_alignment_stats on' in str(e.value)
    # the handle's setting, read when the call is made; another pad id gives other sentence lengths
    eng.set_alignment_stats(True, pad_id=int(c.ids[1, 0]))
    try:
        c.run()
        records = eng.synth_alignment_stats(c.B)
        assert list(records['n_sent']) == list(O.text_lengths(c.ids, int(c.ids[1, 0]))) and records['n_sent'][1] == 1
        with pytest.raises(H.TtsError) as e:
            eng.synth_alignment_stats(c.B + 1)
        assert 'the last call had 3 utterances' in str(e.value)
    finally:
        eng.set_alignment_stats(False)
    assert eng.lib.tts_set_alignment_stats(None, 0, 0) == H.TTS_ERR_INVALID
    assert_same_outputs(c.host(c.run()), c.off)


def test_the_records_do_not_change_with_the_other_settings(case):
    c, eng = case, case.engine
    want = c.by_hand(c.off['alignments'])
    threshold_db = E.choose_threshold(c.off['linear'], c.case['min_frames'])
    assert threshold_db is not None
    for kw in (dict(stop_at_silence=(threshold_db, 0)), dict(speaking_rate=1.25), dict(pitch=UP), dict(loudness=(-23.0, 1e6)),
               dict(stop_at_silence=(threshold_db, 0), speaking_rate=1.25, pitch=UP, loudness=(-23.0, 1e6), momentum=0.99)):
        plain = c.run(**kw)
        out = c.run(on=True, **kw)
        assert O.same_records(eng.synth_alignment_stats(c.B), want), kw
        assert np.array_equal(bits(out['wav'].to_host()), bits(plain['wav'].to_host())), kw
        assert np.array_equal(bits(out['alignments'].to_host()), bits(c.off['alignments'])), kw


def test_local_attention():
    hp = copy.deepcopy(E.hparams_of(E.E2E))
    hp.attention.mechanism = 'LocalLuongAttention'
    hp.attention.luong_local_window_D = 4
    c = Case(E.E2E, hp=hp, weights=pkg('tacotron.weights').synthetic_weights(3, hp))
    try:
        want = c.by_hand(c.off['alignments'])
        for _ in range(2):
            out = c.run(on=True)
            assert O.same_records(c.engine.synth_alignment_stats(c.B), want)
            assert_same_outputs(c.host(out), c.off)
        c.run(on=True, want=False)
        assert O.same_records(c.engine.synth_alignment_stats(c.B), want)
    finally:
        c.engine.close()


# ---------------------------------------------------------------------------------------------- the entry points above
def _model(case):
    M = pkg('tacotron.model')
    return M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.PREDICT, hparams=case.hp, engine=case.engine)


def test_check_alignment_through_synthesize_batch_and_stream(case):
    I = pkg('tacotron.inference')
    A = pkg('tacotron.attention_check')
    model = _model(case)
    want = case.by_hand(case.off['alignments'])
    plain = I.synthesize_batch(model, case.ids, n_steps=case.S, n_iter=3, seed=SEED)
    wavs, records, verdicts = I.synthesize_batch(model, case.ids, n_steps=case.S, n_iter=3, seed=SEED, check_alignment=True)
    assert np.array_equal(bits(wavs), bits(plain)) and O.same_records(records, want)
    assert verdicts == A.verdict(want) and len(verdicts) == case.B and all(set(v) <= set(A.FLAGS) for v in verdicts)
    batches = [case.ids, E.ids_of(case.case, seed=5), case.ids, case.ids]
    items = list(I.synthesize_stream(model, batches, n_steps=case.S, n_iter=3, seed=SEED, copy=True, want_alignments=True, check_alignment=True))
    assert len(items) == 4
    for ids, (w, lin, ali, recs, verd) in zip(batches, items):
        assert lin is None and O.same_records(recs, case.by_hand(ali, ids)) and verd == A.verdict(recs)
    assert O.same_records(items[0][3], want)
    items = list(I.synthesize_stream(model, batches[:2], n_steps=case.S, n_iter=3, seed=SEED, copy=True, check_alignment=True))
    assert [len(i) for i in items] == [3, 3] and O.same_records(items[0][1], want)
    plain = list(I.synthesize_stream(model, batches[:2], n_steps=case.S, n_iter=3, seed=SEED, copy=True))
    assert all(np.array_equal(bits(a[0]), bits(b)) for a, b in zip(items, plain))


@pytest.mark.parametrize('pipelined', [False, True])
def test_check_alignment_through_serve(weights, pipelined):
    S = pkg('tacotron.serve')
    P = pkg('tacotron.params')
    A = pkg('tacotron.attention_check')
    requests = [['Hello there.', 'Hi'], ['One more.']]
    P.model_params.decoder.maximum_iterations = 20
    P.model_params.reconstruction_iterations = 2
    try:
        plain = list(S.serve(iter(requests), weights, pipelined=pipelined))
        checked = list(S.serve(iter(requests), weights, pipelined=pipelined, check_alignment=True))
    finally:
        P.model_params.decoder.maximum_iterations = 1000
        P.model_params.reconstruction_iterations = 50
    assert len(checked) == 2
    for (wavs, records, verdicts), before, sentences in zip(checked, plain, requests):
        assert len(wavs) == len(records) == len(verdicts) == len(sentences)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(wavs, before))
        assert verdicts == A.verdict(records) and np.all(records['n_steps'] == 20 // P.model_params.reduction)
    ds = pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)
    for (wavs, records, verdicts), sentences in zip(checked, requests):
        assert list(records['n_sent']) == list(O.text_lengths(S.pre_process_sentences(sentences, ds), 0))
    assert list(checked[0][1]['n_sent']) == [12, 3]                      # (the characters the front end keeps, and the end token)


def test_the_command_line_report(case, tmp_path, monkeypatch, capsys):
    I = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', 20)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    sentences = tmp_path / 'sentences.txt'
    sentences.write_text('Hello there.\nHi\n')
    out_dir = tmp_path / 'out'
    out_dir.mkdir()
    assert I.main(['--synthesis-file', str(sentences), '--synthesis-dir', str(out_dir), '--synthetic-weights', '0', '--check-alignment']) == 0
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith('{')]
    assert [row['index'] for row in lines] == [0, 1] and all(set(row) == {'index', 'verdict', 'record'} for row in lines)
    with open(os.path.join(str(out_dir), I.REPORT_FILE)) as f:
        assert json.load(f) == lines
    assert sorted(os.listdir(str(out_dir))) == ['1.wav', '2.wav', I.REPORT_FILE]
    assert [row['record']['n_sent'] for row in lines] == [12, 3] and all(row['record']['n_steps'] == 4 for row in lines)


# ---------------------------------------------------------------------------------------------- gta
def test_gta_files_carry_the_record_and_the_kernels_durations_are_gta_durations(engine, hparams, tmp_path, monkeypatch):
    G = pkg('tacotron.gta')
    P = pkg('tacotron.params')
    M = pkg('tacotron.model')
    H = pkg('_hip')
    monkeypatch.setattr(P.evaluation_params, 'n_buckets', 2)
    r, nm, F = hparams.reduction, hparams.n_mels, 1 + hparams.n_fft // 2
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'wavs'))
    rows = [('LJ00{}'.format(i), text) for i, text in enumerate(['a cat', 'hi there', 'a longer sentence', 'dogs', 'the end'])]
    rng = np.random.default_rng(0)
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for i, (fid, text) in enumerate(rows):
            f.write('{}|{}|{}\n'.format(fid, text.upper(), text))
            np.savez(os.path.join(root, 'wavs', fid + '.npz'), mel_mag_db=rng.random((2 + i % 4, nm * r)).astype(np.float32),
                     linear_mag_db=rng.random((2 + i % 4, F * r)).astype(np.float32))
    dataset = pkg('datasets.lj_speech').LJSpeechDatasetHelper(root, P.dataset_params.vocabulary_dict, False)
    model = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.PREDICT, hparams=hparams, engine=engine)
    out_dir = str(tmp_path / 'gta')
    res = G.write_gta(model, G.batches_with_paths(dataset, None, 3, verbose=False), out_dir, verbose=False, attention_stats=True)
    assert res['n_files'] == len(rows)
    for fid, _ in rows:
        with np.load(os.path.join(out_dir, fid + '.gta.npz')) as z:
            assert set(z.files) == {'mel_mag_db', 'alignments', 'durations', 'attention_stats'}
            rec, ali = z['attention_stats'], z['alignments']
            assert rec.dtype == H.ALIGNMENT_RECORD and rec.shape == ()
            # the record of the cropped alignments: the padding of the batch is read for off_text alone
            want = O.utterance(ali, ali.shape[1])[0]
            for field in O.FIELDS:
                if field != 'off_text':
                    assert rec[field] == want[field], (fid, field)
            assert rec['focus_sum'].view(np.uint64) == np.float64(want['focus_sum']).view(np.uint64)
            # ... and the kernel's durations, times r, are gta.durations
            _stats, dur = engine.alignment_stats(np.ascontiguousarray(ali[:, None, :]), want_durations=True)
            assert np.array_equal(dur[0] * r, z['durations']) and np.array_equal(z['durations'], G.durations(ali, r))
