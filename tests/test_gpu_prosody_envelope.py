"""GPU: ``tacotron.inference.synthesize_marked(markup_pitch=True, pitch_mode='envelope')`` against the test's own composition of the
same stages, bit for bit, in the setup of tests/test_gpu_prosody.py (cudnn-narrow, B = 3 sentences, 12 decoder steps, 2 iterations):
the shift runs between denorm_power and the warp and nothing is resampled; row lengths and marks are those of the same text with
the pitch attributes removed; a call with the option and nothing to shift against the call without it; the global ``pitch`` and
``timbre``; ``--pitch-mode`` and ``--timbre`` through ``main()``."""
import os

import numpy as np
import pytest

import test_gpu_prosody as G
from conftest import pkg
from test_gpu_prosody import dataset, model   # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

S, N_ITER, SEED, PLAIN = G.S, G.N_ITER, G.SEED, G.PLAIN
WORDS = [[(0, 3), (4, 7), (8, 11)], [(0, 1), (2, 5), (6, 9)]]     # of PLAIN[0] and PLAIN[1]


def _texts(start):
    """``(with pitch, the same without)``: the word of sentence 0 that the alignment gives the most decoder steps four semitones up
    at 80 % of the rate, the one of sentence 1 three semitones down and 6 dB softer behind a 200 ms break, sentence 2 as it is"""
    marked, bare = [], []
    for b, (pitch, rest, lead) in enumerate((('+4st', 'rate="80%"', ''), ('-3st', 'volume="-6 dB"', '<break time="200ms"/>'))):
        n = [int(start[b][j] - start[b][i]) for i, j in WORDS[b]]
        assert max(n) >= 1
        i, j = WORDS[b][int(np.argmax(n))]
        for out, attrs in ((marked, 'pitch="{}" {}'.format(pitch, rest)), (bare, rest)):
            out.append(PLAIN[b][:i] + lead + '<prosody {}>'.format(attrs) + PLAIN[b][i:j] + '</prosody>' + PLAIN[b][j:])
    return marked + [PLAIN[2]], bare + [PLAIN[2]]


def _composition(model, dataset, marked, pitch=0.0, timbre=0.0, stop=None):
    """the stages, composed here: ``(waveforms, shift segments per row)``"""
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.prosody')
    hp, eng = model.hparams, model.engine
    win, hop, min_frames = G._shape(model)
    s = inf.SynthSettings(model, stop_at_silence_db=stop, silence_keep_ms=0.0)
    mag, start, n_sent, n_frames = G._network(model, dataset, PLAIN, s.stop)
    segments, n_out, shift, per_row = [], [], [], []
    for b, text in enumerate(marked):
        plain, spans, breaks = P.parse_markup(text, pitch=True)
        attrs, tb = P.token_attributes(dataset, plain, spans, breaks, 1.0, hop, hp.sampling_rate, pitch=True, pitch_mode='envelope')
        cut, _n, st = P.segments_of_row(start[b], int(n_sent[b]), hp.reduction, int(n_frames[b]), attrs, tb, min_frames, row=b)
        per_row.append(P.shift_segments_of_row(cut, [0.0 if q[2] == 0 else v + 12.0 * pitch for q, v in zip(cut, st)], timbre, row=b))
        seg, n = P.segments_of_row(start[b], int(n_sent[b]), hp.reduction, int(n_frames[b]), [a[:2] for a in attrs], tb, min_frames, row=b)   # the warp's: no pitch
        shift += per_row[-1]
        segments += seg
        n_out.append(n)
    shifted = eng.shift_magnitudes(mag, shift, n_frames)
    warped, got_n = eng.warp_magnitudes(shifted, segments, n_frames)
    assert got_n.tolist() == n_out
    wav, _mse = eng.griffin_lim(warped, N_ITER, win, hop, hp.n_fft, seed=SEED, want_mse=False, n_frames=n_out)
    try:
        host = wav.to_host()
        return [host[b, :hop * (n - 1)] for b, n in enumerate(n_out)], per_row
    finally:
        for a in (mag, shifted, warped, wav):
            a.free()


@pytest.mark.parametrize('stop', [None, -40.0])
def test_it_is_the_stages_with_the_shift_and_lengths_and_marks_are_those_without_a_pitch(model, dataset, stop):
    inf = pkg('tacotron.inference')
    H = pkg('_hip')
    marked, bare = _texts(G._network(model, dataset, PLAIN)[1])
    kw = dict(n_iter=N_ITER, seed=SEED, marks='word', want_plan=True, stop_at_silence_db=stop, silence_keep_ms=0.0)
    wavs, marks, plan = inf.synthesize_marked(model, marked, dataset, markup_pitch=True, pitch_mode='envelope', **kw)
    want, per_row = _composition(model, dataset, marked, stop=stop)
    G._same(wavs, want)
    assert plan['shift_segments'] == per_row and plan['pitch_segments'] is None
    steps = [{q[3] for q in seg} for seg in per_row]
    assert H.shift_step(4.0) in steps[0] <= {65536, H.shift_step(4.0)} and H.shift_step(-3.0) in steps[1] <= {65536, H.shift_step(-3.0)}
    assert steps[2] == {65536} and all(q[4] == 65536 for seg in per_row for q in seg)
    # the same text with the pitch attributes removed: the same rows lengths, the same marks, other samples
    plain_wavs, plain_marks, plain_plan = inf.synthesize_marked(model, bare, dataset, **kw)
    assert [len(w) for w in wavs] == [len(w) for w in plain_wavs] == plan['n_samples'] and plan['n_out'] == plain_plan['n_out']
    assert plan['segments'] == plain_plan['segments'] and marks == plain_marks and 'shift_segments' not in plain_plan
    assert not np.array_equal(wavs[0], plain_wavs[0]) and not np.array_equal(wavs[1], plain_wavs[1])
    assert np.array_equal(wavs[2].view(np.uint32), plain_wavs[2].view(np.uint32))                # a row without a pitch: copies, the same bits


def test_nothing_to_shift_gives_the_bits_of_the_call_without_the_option(model, dataset):
    inf = pkg('tacotron.inference')
    eng = model.engine
    _marked, bare = _texts(G._network(model, dataset, PLAIN)[1])
    kw = dict(n_iter=N_ITER, seed=SEED, marks='word', want_plan=True)
    eng.set_option('profile', 1)
    try:
        for texts in (PLAIN, bare, [bare[0], '<prosody pitch="+0.1st">a cat</prosody> sat', '<prosody pitch="medium">go</prosody> on']):
            base = [t if 'pitch' not in t else PLAIN[b] for b, t in enumerate(texts)]
            want, want_marks, want_plan = inf.synthesize_marked(model, base, dataset, **kw)
            eng.profile_reset()
            got, got_marks, got_plan = inf.synthesize_marked(model, texts, dataset, markup_pitch=True, pitch_mode='envelope', pitch=0.0, timbre=0.0, **kw)
            assert eng.profile_get('shift') == (0.0, 0)                                           # the stage is not launched
            G._same(got, want)
            assert got_marks == want_marks and got_plan['shift_segments'] is None and got_plan['segments'] == want_plan['segments']
    finally:
        eng.set_option('profile', 0)


def test_the_global_pitch_and_the_timbre_are_taken_here_and_refused_in_the_default_mode(model, dataset):
    inf = pkg('tacotron.inference')
    H = pkg('_hip')
    marked, _bare = _texts(G._network(model, dataset, PLAIN)[1])
    got, plan = inf.synthesize_marked(model, marked, dataset, n_iter=N_ITER, seed=SEED, want_plan=True, markup_pitch=True, pitch_mode='envelope',
                                      pitch=2.0 / 12.0, timbre=-1.5)
    want, per_row = _composition(model, dataset, marked, pitch=2.0 / 12.0, timbre=-1.5)
    G._same(got, want)
    assert plan['shift_segments'] == per_row
    # (synthetic weights align as they please: the other words of sentence 0 may own no frame at all)
    assert {H.shift_step(6.0)} <= {q[3] for q in per_row[0]} <= {H.shift_step(2.0), H.shift_step(6.0)} and {q[3] for q in per_row[2]} == {H.shift_step(2.0)}
    assert {q[4] for seg in per_row for q in seg} == {H.shift_step(-1.5)}
    # a text without a pitch: the global one alone launches the stage
    alone, plan = inf.synthesize_marked(model, PLAIN, dataset, n_iter=N_ITER, seed=SEED, want_plan=True, markup_pitch=True, pitch_mode='envelope', pitch=-0.25)
    assert [[q[3:] for q in seg] for seg in plan['shift_segments']] == [[(H.shift_step(-3.0), 65536)]] * 3
    assert all(np.isfinite(w).all() and np.abs(w).max() > 0 for w in alone)
    # a border between two pitches alone does not cut the warp's segments: at a base rate of 0.8, where every segment rounds up to a
    # whole frame, the rows are as long as without the pitch
    kw = dict(n_iter=N_ITER, seed=SEED, want_plan=True, speaking_rate=0.8)
    _w, with_pitch = inf.synthesize_marked(model, PLAIN[:2] + ['<prosody pitch="+2st">go</prosody> on'], dataset, markup_pitch=True, pitch_mode='envelope', **kw)
    _w, without = inf.synthesize_marked(model, PLAIN, dataset, **kw)
    assert with_pitch['n_out'] == without['n_out'] and with_pitch['segments'] == without['segments']
    assert {q[3] for q in with_pitch['shift_segments'][2]} <= {65536, H.shift_step(2.0)} and 'shift_segments' not in without
    for kw in (dict(markup_pitch=True, pitch=0.25), dict(pitch=0.25), dict(markup_pitch=True, timbre=1.0), dict(pitch_mode='envelope'),
               dict(markup_pitch=True, pitch_mode='envelope', pitch=0.75)):                       # (+4 st and +9 st: more than an octave)
        with pytest.raises(ValueError):
            inf.synthesize_marked(model, marked if kw.get('markup_pitch') else PLAIN, dataset, n_iter=N_ITER, **kw)


def test_the_flags_through_main(tmp_path, monkeypatch):
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    io = pkg('audio.io')
    lines = ['<prosody pitch="+4st">one two</prosody> six', 'a cat <break time="200ms"/>sat', '<prosody pitch="low">go</prosody> on']
    (tmp_path / 'sentences.txt').write_text('\n'.join(lines) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', 4 * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    common = ['--synthesis-file', str(tmp_path / 'sentences.txt'), '--synthesis-dir', str(out), '--synthetic-weights', '0']
    assert inf.main(common + ['--markup', '--markup-pitch', '--pitch-mode', 'envelope', '--pitch', '1', '--timbre', '-2']) == 0
    assert sorted(os.listdir(out)) == ['1.wav', '2.wav', '3.wav']
    for i in range(3):
        wav, sr = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert sr == 22050 and np.isfinite(wav).all() and len(wav) == 275 * (20 + (16 if i == 1 else 0) - 1)   # whole hops: nothing is resampled
    for bad in (['--pitch-mode', 'envelope'], ['--markup', '--pitch-mode', 'envelope'], ['--markup', '--markup-pitch', '--timbre', '1'],
                ['--markup', '--markup-pitch', '--pitch', '2'], ['--markup', '--markup-pitch', '--pitch-mode', 'envelope', '--timbre', '13']):
        with pytest.raises(SystemExit) as e:
            inf.main(common + bad)
        assert e.value.code == 2
