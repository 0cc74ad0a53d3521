"""GPU: ``tacotron.inference.synthesize_marked`` against the test's own composition of the same stages, bit for bit, with synthetic
weights at the smallest architecture of tests/arch_cases.py that takes the text front end's vocabulary (cudnn-narrow: n_mels 16,
r = 2), B = 3 sentences and 12 decoder steps; the silence of a break at a small n_fft of the general kernels; ``--markup`` through
``main()``."""
import json
import os
import types

import numpy as np
import pytest

import arch_cases as A
from conftest import pkg

pytestmark = pytest.mark.gpu

S, N_ITER, SEED = 12, 2, 5
PLAIN = ['one two six', 'a cat sat', 'go on']
WORDS = [(0, 3), (4, 7), (8, 11)]     # of PLAIN[0]


def _marked(start):
    """PLAIN with the word of sentence 0 that the alignment gives the most decoder steps at half the rate (synthetic weights align
    as they please: a word without a step would leave the warp nothing to slow) and a 200 ms break in sentence 1"""
    steps = [int(start[0][b] - start[0][a]) for a, b in WORDS]
    a, b = WORDS[int(np.argmax(steps))]
    return [PLAIN[0][:a] + '<prosody rate="50%">' + PLAIN[0][a:b] + '</prosody>' + PLAIN[0][b:], 'a cat <break time="200ms"/>sat', 'go on'], max(steps)


@pytest.fixture(scope='module')
def model():
    hp, w, _ = A.arch('cudnn-narrow')
    eng = pkg().Engine(hp)
    eng.load_weights(w)
    yield types.SimpleNamespace(hparams=hp, engine=eng, n_steps=lambda: S)
    eng.close()


@pytest.fixture(scope='module')
def dataset():
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)


def _shape(model):
    conv = pkg('audio.conversion')
    hp = model.hparams
    win, hop = conv.ms_to_samples(hp.win_len, hp.sampling_rate), conv.ms_to_samples(hp.win_hop, hp.sampling_rate)
    return win, hop, (hp.n_fft // 2) // hop + 2      # (Griffin-Lim's least: hop (n - 1) > n_fft / 2)


def _network(model, dataset, sentences, stop=None):
    """the stages in front of the warp, composed here: ``(mag, start, n_sent, n_frames)``"""
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    hp, eng = model.hparams, model.engine
    loader = P.dataset_params.dataset_loader
    seqs, n_sent = dataset.process_sentences(sentences)
    ids = np.array([inf.pad_sentence(np.frombuffer(q, dtype=np.int32), max(n_sent)) for q in seqs], dtype=np.int32)
    mem = eng.encoder_forward(ids)
    mel, ali = eng.decoder_forward(mem, S)
    start, _stats = eng.token_times(ali, n_sent=np.asarray(n_sent, np.int32), max_jump=4)
    mel.shape = (len(sentences), S * hp.reduction, hp.n_mels)
    lin = eng.postnet_forward(mel)
    n_frames = np.full(len(sentences), S * hp.reduction, np.int32)
    if stop is not None:
        _win, hop, min_frames = _shape(model)
        d, _last = eng.speech_frames(lin, eng.speech_threshold(stop[0], loader.mel_mag_ref_db, loader.mel_mag_max_db), stop[1], min_frames)
        n_frames = d.to_host().astype(np.int32)
    mag = eng.denorm_power(lin, loader.mel_mag_ref_db, loader.mel_mag_max_db, hp.magnitude_power)
    return mag, start, np.asarray(n_sent, np.int32), n_frames


def _griffin_lim(model, mag, n_frames):
    win, hop, _m = _shape(model)
    wav, _mse = model.engine.griffin_lim(mag, N_ITER, win, hop, model.hparams.n_fft, seed=SEED, want_mse=False, n_frames=n_frames)
    host = wav.to_host()
    return [host[b, :hop * (int(n) - 1)] for b, n in enumerate(n_frames)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.isfinite(g).all() and np.abs(g).max() > 0


def test_without_markup_it_is_the_stages_without_the_warp(model, dataset):
    inf = pkg('tacotron.inference')
    got, plan = inf.synthesize_marked(model, PLAIN, dataset, n_iter=N_ITER, seed=SEED, want_plan=True)
    mag, start, n_sent, n_frames = _network(model, dataset, PLAIN)
    T = S * model.hparams.reduction
    assert plan['n_out'] == [T] * 3 and [len(s) for s in plan['segments']] == [1, 1, 1] and np.array_equal(plan['start'], start)
    assert plan['plain'] == PLAIN
    _same(got, _griffin_lim(model, mag, n_frames))


@pytest.mark.parametrize('stop', [None, -40.0])
def test_with_markup_it_is_the_stages_with_the_warp_and_the_marks_go_through_it(model, dataset, stop):
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    hp, eng = model.hparams, model.engine
    win, hop, min_frames = _shape(model)
    MARKED, slowed_steps = _marked(_network(model, dataset, PLAIN)[1])
    assert slowed_steps >= 1
    wavs, marks, plan = inf.synthesize_marked(model, MARKED, dataset, n_iter=N_ITER, seed=SEED, marks='word', want_plan=True,
                                              stop_at_silence_db=stop, silence_keep_ms=0.0)
    s = inf.SynthSettings(model, stop_at_silence_db=stop, silence_keep_ms=0.0)
    mag, start, n_sent, n_frames = _network(model, dataset, PLAIN, s.stop)
    assert plan['plain'] == PLAIN and np.array_equal(plan['start'], start) and np.array_equal(plan['n_frames'], n_frames)
    # every row's length: segments_of_row applied to the start the call itself reports
    segments, n_out = [], []
    for b, text in enumerate(MARKED):
        plain, spans, breaks = P.parse_markup(text)
        attrs, tb = P.token_attributes(dataset, plain, spans, breaks, 1.0, hop, hp.sampling_rate)
        seg, n = P.segments_of_row(plan['start'][b], int(n_sent[b]), hp.reduction, int(n_frames[b]), attrs, tb, min_frames, row=b)
        assert seg == plan['segments'][b] and n == plan['n_out'][b]
        segments += seg
        n_out.append(n)
    assert [len(w) for w in wavs] == [hop * (n - 1) for n in n_out]
    if stop is None:
        assert any(q[4] == 32768 for q in segments if q[0] == 0) and n_out[0] == (S + slowed_steps) * hp.reduction      # the slowed word
        assert (1, 0, 0, 16, 0, 0.0) in segments and n_out[1] == S * hp.reduction + 16 and n_out[2] == S * hp.reduction   # the break: 200 ms
    warped, got_n = eng.warp_magnitudes(mag, segments, n_frames)
    assert got_n.tolist() == n_out
    _same(wavs, _griffin_lim(model, warped, n_out))
    # the marks: marks_of_row through warp_position
    for b, plain in enumerate(PLAIN):
        processed, tok = M.token_spans(dataset, plain)
        seg = plan['segments'][b]
        want = M.marks_of_row(processed, tok, plan['start'][b], hp.reduction, hop, 1.0, hop * (int(n_frames[b]) - 1), hp.sampling_rate, None,
                              len(wavs[b]), 'word', raw=plain, place=lambda x, seg=seg: hop * P.warp_position(seg, x / hop, 'right'),
                              place_end=lambda x, seg=seg: hop * P.warp_position(seg, x / hop, 'left'))
        got = [{k: v for k, v in m.items() if k != 'reliable'} for m in marks[b]]
        assert got == want and [m['value'] for m in got if m['type'] == 'word'] == plain.split()
        assert all(0 <= m['sample'] <= m['end_sample'] <= len(wavs[b]) for m in got)


def test_a_pitch_is_refused(model, dataset):
    inf = pkg('tacotron.inference')
    with pytest.raises(ValueError, match='pitch'):
        inf.synthesize_marked(model, PLAIN, dataset, pitch=0.25)


def test_a_break_is_silence(engine):
    """Samples more than n_fft / 2 from the centre of every frame that is not a pause's are exactly zero: a pause's frames are
    +0.0, so every product with them is, and the overlap-add of zeros is zero.  n_fft 256 of the general kernels, hop 64."""
    n_fft, hop, F, T = 256, 64, 129, 12
    rng = np.random.default_rng(3)
    mag = rng.random((2, F, T)).astype(np.float32) + 0.1
    seg = [(0, 0, 6, 0, 65536, 1.0), (0, 0, 0, 12, 0, 0.0), (0, 6, 6, 0, 32768, 1.0), (1, 0, 12, 0, 65536, 1.0)]
    warped, n_out = engine.warp_magnitudes(mag, seg)
    assert n_out.tolist() == [30, 12]
    wav, _mse = engine.griffin_lim(warped, 3, n_fft, hop, n_fft, seed=1, want_mse=False, n_frames=n_out.tolist())
    host = wav.to_host()
    warped.free()
    wav.free()
    centres = np.array([t * hop for t in range(30) if not 6 <= t < 18])
    far = np.array([np.abs(centres - i).min() > n_fft // 2 for i in range(hop * 29)])
    assert far.sum() == (18 * hop - n_fft // 2) - (5 * hop + n_fft // 2) - 1 == 575              # samples 449 .. 1023
    quiet = host[0, :hop * 29] == 0                                                             # exactly zero (either sign)
    assert quiet[far].all() and (~quiet[:hop * 4]).any() and (~quiet[hop * 20:]).any()
    assert not (host[1, :hop * 11] == 0).all()


def test_markup_through_main(tmp_path, monkeypatch):
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    io = pkg('audio.io')
    (tmp_path / 'sentences.txt').write_text('\n'.join(_marked([[0, 1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13]])[0]) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', 4 * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    assert inf.main(['--synthesis-file', str(tmp_path / 'sentences.txt'), '--synthesis-dir', str(out), '--synthetic-weights', '0', '--markup',
                     '--marks']) == 0
    assert sorted(os.listdir(out)) == ['1.marks.jsonl', '1.wav', '2.marks.jsonl', '2.wav', '3.marks.jsonl', '3.wav']
    lengths = []
    for i, plain in enumerate(PLAIN):
        wav, sr = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert sr == 22050 and np.isfinite(wav).all() and len(wav) % 275 == 0
        lengths.append(len(wav) // 275 + 1)
        with open(out / '{}.marks.jsonl'.format(i + 1)) as f:
            marks = [json.loads(line) for line in f]
        assert marks[0]['type'] == 'sentence' and [m['value'] for m in marks if m['type'] == 'word'] == plain.split()
        assert all(plain[m['start']:m['end']] == m['value'] for m in marks)                      # offsets into the line with the markup removed
    assert lengths[1] == 20 + 16 and lengths[2] == 20 and lengths[0] >= 20                       # the break's 16 frames; a slowed word adds frames
    for bad in (['--markup', '--text'], ['--markup', '--pitch', '2']):
        with pytest.raises(SystemExit) as e:
            inf.main(['--synthesis-file', str(tmp_path / 'sentences.txt'), '--synthesis-dir', str(out)] + bad)
        assert e.value.code == 2
