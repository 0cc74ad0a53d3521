"""GPU: ``tacotron.inference.synthesize_marked(markup_pitch=True)`` against the test's own composition of the same stages, bit for
bit, in the setup of tests/test_gpu_prosody.py (cudnn-narrow, B = 3 sentences, 12 decoder steps, 2 iterations); the marks through
both maps; a call with the option and no pitch against the call without it; ``--markup --markup-pitch`` through ``main()``; and one
test that listens: a tone through ``Engine.resample_segments``, tracked by ``Engine.f0``."""
import json
import os

import numpy as np
import pytest

import f0_cases as K
import test_gpu_prosody as G
from conftest import pkg
from test_gpu_prosody import dataset, model   # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

S, N_ITER, SEED, PLAIN = G.S, G.N_ITER, G.SEED, G.PLAIN
WORDS = [[(0, 3), (4, 7), (8, 11)], [(0, 1), (2, 5), (6, 9)]]     # of PLAIN[0] and PLAIN[1]


def _marked(start):
    """PLAIN with the word of sentence 0 that the alignment gives the most decoder steps four semitones up, the one of sentence 1
    three semitones down at 80 % of the rate behind a 200 ms break, and sentence 2 as it is (synthetic weights align as they
    please: a word without a step would leave nothing to shift)"""
    out, steps = [], []
    for b, (open_, close) in enumerate((('<prosody pitch="+4st">', '</prosody>'), ('<break time="200ms"/><prosody pitch="-3st" rate="80%">', '</prosody>'))):
        n = [int(start[b][j] - start[b][i]) for i, j in WORDS[b]]
        i, j = WORDS[b][int(np.argmax(n))]
        out.append(PLAIN[b][:i] + open_ + PLAIN[b][i:j] + close + PLAIN[b][j:])
        steps.append(max(n))
    return out + [PLAIN[2]], steps


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.isfinite(g).all() and np.abs(g).max() > 0


@pytest.mark.parametrize('stop', [None, -40.0])
def test_with_a_pitch_it_is_the_stages_with_the_pass_and_the_marks_go_through_both_maps(model, dataset, stop):
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.prosody')
    M = pkg('tacotron.marks')
    hp, eng = model.hparams, model.engine
    win, hop, min_frames = G._shape(model)
    MARKED, shifted_steps = _marked(G._network(model, dataset, PLAIN)[1])
    assert min(shifted_steps) >= 1
    wavs, marks, plan = inf.synthesize_marked(model, MARKED, dataset, n_iter=N_ITER, seed=SEED, marks='word', want_plan=True, markup_pitch=True,
                                              stop_at_silence_db=stop, silence_keep_ms=0.0)
    s = inf.SynthSettings(model, stop_at_silence_db=stop, silence_keep_ms=0.0)
    mag, start, n_sent, n_frames = G._network(model, dataset, PLAIN, s.stop)
    assert plan['plain'] == PLAIN and np.array_equal(plan['start'], start) and np.array_equal(plan['n_frames'], n_frames)
    segments, n_out, psegs, per_row = [], [], [], []
    for b, text in enumerate(MARKED):
        plain, spans, breaks = P.parse_markup(text, pitch=True)
        attrs, tb = P.token_attributes(dataset, plain, spans, breaks, 1.0, hop, hp.sampling_rate, pitch=True)
        seg, n, ratios = P.segments_of_row(plan['start'][b], int(n_sent[b]), hp.reduction, int(n_frames[b]), attrs, tb, min_frames, row=b)
        pseg, n_new = P.pitch_segments_of_row(seg, ratios, hop, n, row=b)
        assert seg == plan['segments'][b] and n == plan['n_out'][b] and pseg == plan['pitch_segments'][b] and n_new == plan['n_samples'][b]
        segments += seg
        n_out.append(n)
        psegs += pseg
        per_row.append((seg, pseg))
    assert [len(w) for w in wavs] == plan['n_samples']
    if stop is None:
        up, down = 2.0 ** (-4.0 / 12.0), 2.0 ** (3.0 / 12.0)
        assert up in {q[3] for q in per_row[0][1]} <= {1.0, up} and down in {q[3] for q in per_row[1][1]} <= {1.0, down}
        assert per_row[2][1] == [(2, 0, hop * (n_out[2] - 1), 1.0)]                              # a row without a pitch: one copy
        # the rows last what they last unshifted: the warp rounds a segment up to a whole frame with and without the pitch (up to
        # hop * ratio < 2 hop samples more, up to hop fewer), and the pass truncates less than a sample per segment
        plain_n = [S * hp.reduction, S * hp.reduction + 16 + int(np.ceil(shifted_steps[1] * hp.reduction / 0.8)) - shifted_steps[1] * hp.reduction,
                   S * hp.reduction]
        for b in range(3):
            assert -hop - len(per_row[b][1]) < plan['n_samples'][b] - hop * (plain_n[b] - 1) < hop * 2 + len(per_row[b][1])
    warped, got_n = eng.warp_magnitudes(mag, segments, n_frames)
    assert got_n.tolist() == n_out
    wav, _mse = eng.griffin_lim(warped, N_ITER, win, hop, hp.n_fft, seed=SEED, want_mse=False, n_frames=n_out)
    held = hop * (np.asarray(n_out, np.int32) - 1)
    retimed, n_new = eng.resample_segments(wav, psegs, held)
    try:
        assert n_new.tolist() == plan['n_samples']
        host, gl = retimed.to_host(), wav.to_host()
        _same(wavs, [host[b, :int(n)] for b, n in enumerate(n_new)])
        assert np.array_equal(wavs[2].view(np.uint32), gl[2, :held[2]].view(np.uint32))           # ... and it keeps Griffin-Lim's bits
    finally:
        for a in (warped, wav, retimed, mag):
            a.free()
    # the marks: marks_of_row through pitch_position(hop * warp_position(..))
    for b, plain in enumerate(PLAIN):
        processed, tok = M.token_spans(dataset, plain)
        seg, pseg = per_row[b]
        want = M.marks_of_row(processed, tok, plan['start'][b], hp.reduction, hop, 1.0, hop * (int(n_frames[b]) - 1), hp.sampling_rate, None,
                              len(wavs[b]), 'word', raw=plain,
                              place=lambda x, seg=seg, pseg=pseg: P.pitch_position(pseg, hop * P.warp_position(seg, x / hop, 'right'), 'right'),
                              place_end=lambda x, seg=seg, pseg=pseg: P.pitch_position(pseg, hop * P.warp_position(seg, x / hop, 'left'), 'left'))
        got = [{k: v for k, v in m.items() if k != 'reliable'} for m in marks[b]]
        assert got == want and [m['value'] for m in got if m['type'] == 'word'] == plain.split()
        assert all(0 <= m['sample'] <= m['end_sample'] <= len(wavs[b]) for m in got)


def test_without_a_pitch_in_the_text_the_option_changes_nothing(model, dataset):
    inf = pkg('tacotron.inference')
    marked = G._marked(G._network(model, dataset, PLAIN)[1])[0]                                   # a slowed word and a break, no pitch
    for texts in (PLAIN, marked, [marked[0], '<prosody pitch="+0.1st">a cat</prosody> sat', '<prosody pitch="medium">go</prosody> on']):
        base = [t if 'pitch' not in t else PLAIN[b] for b, t in enumerate(texts)]
        want, want_marks, want_plan = inf.synthesize_marked(model, base, dataset, n_iter=N_ITER, seed=SEED, marks='word', want_plan=True)
        got, got_marks, got_plan = inf.synthesize_marked(model, texts, dataset, n_iter=N_ITER, seed=SEED, marks='word', want_plan=True, markup_pitch=True)
        _same(got, want)
        assert got_marks == want_marks and got_plan['pitch_segments'] is None
        assert got_plan['n_samples'] == [len(w) for w in want] and got_plan['segments'] == want_plan['segments']
        assert 'pitch_segments' not in want_plan and 'n_samples' not in want_plan
    with pytest.raises(ValueError, match='pitch'):
        inf.synthesize_marked(model, PLAIN, dataset, markup_pitch=True, pitch=0.25)
    with pytest.raises(ValueError, match='unknown attribute pitch='):
        inf.synthesize_marked(model, ['<prosody pitch="+2st">go</prosody> on'], dataset)


def test_markup_pitch_through_main(tmp_path, monkeypatch):
    inf = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    io = pkg('audio.io')
    lines = ['<prosody pitch="+4st">one two</prosody> six', 'a cat <break time="200ms"/>sat', '<prosody pitch="low">go</prosody> <prosody pitch="-10%">on</prosody>']
    (tmp_path / 'sentences.txt').write_text('\n'.join(lines) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', 4 * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    common = ['--synthesis-file', str(tmp_path / 'sentences.txt'), '--synthesis-dir', str(out), '--synthetic-weights', '0']
    assert inf.main(common + ['--markup', '--markup-pitch', '--marks']) == 0
    assert sorted(os.listdir(out)) == ['1.marks.jsonl', '1.wav', '2.marks.jsonl', '2.wav', '3.marks.jsonl', '3.wav']
    for i, plain in enumerate(PLAIN):
        wav, sr = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert sr == 22050 and np.isfinite(wav).all() and len(wav) > 0
        if i == 1:
            assert len(wav) == 275 * (20 + 16 - 1)                                                # no pitch in the line: the break's 16 frames, whole hops
        with open(out / '{}.marks.jsonl'.format(i + 1)) as f:
            marks = [json.loads(line) for line in f]
        assert marks[0]['type'] == 'sentence' and [m['value'] for m in marks if m['type'] == 'word'] == plain.split()
        assert all(plain[m['start']:m['end']] == m['value'] for m in marks) and all(m['end_sample'] <= len(wav) for m in marks)
    for bad in (['--markup-pitch'], ['--markup', '--markup-pitch', '--pitch', '2'], ['--markup', '--pitch', '2']):
        with pytest.raises(SystemExit) as e:
            inf.main(common + bad)
        assert e.value.code == 2
    with pytest.raises(ValueError, match='unknown attribute pitch='):                            # the markup alone still refuses a pitch
        inf.main(common + ['--markup'])


def test_a_tone_comes_out_at_the_pitch_of_its_segment(engine):
    """A 150 Hz harmonic tone of 16 500 samples as three segments at ratios 1, 2 ** (-4 / 12) and 1: the frames of tts_f0 that lie
    wholly inside the middle segment read 150 * 2 ** (4 / 12) Hz, the outer ones 150 Hz -- the median voiced f0 of each part
    against the tracker's own reading of the tone, within 1e-3, the bound tests/test_gpu_f0_pitch.py holds tts_resample to on a
    tone (twice the sum of the tracker's worst errors on two tones)."""
    E = K.EVAL
    hz, n = 150.0, 60 * E['hop']
    x = K.tone(hz, n, seed=150)
    ratio = 2.0 ** (-4.0 / 12.0)
    a, b = 18 * E['hop'], 48 * E['hop']
    seg = [(0, 0, a, 1.0), (0, a, b - a, ratio), (0, b, n - b, 1.0)]

    def track(wav):
        f0 = engine.f0(wav, K.SR, E['hop'], window=E['W'], tau_min=E['tau_min'], tau_max=E['tau_max'])
        out = f0.to_host().copy().reshape(-1)
        f0.free()
        return out

    def median(f0):
        v = f0[f0 > 0]
        assert v.size >= max(1, f0.size // 2)
        return float(np.median(v.astype(np.float64)))

    before = median(track(x))
    out, n_out = engine.resample_segments(x[None], seg)
    y = out.to_host()[0]
    out.free()
    mid = int((b - a) * ratio)
    assert n_out.tolist() == [a + mid + n - b] and np.array_equal(y[:a], x[:a]) and np.array_equal(y[a + mid:], x[b:])
    f0 = track(y)
    half = (E['W'] + E['tau_max']) // 2
    lo = np.array([t * E['hop'] - half for t in range(f0.size)])
    hi = lo + E['W'] + E['tau_max']
    parts = {'first': (lo >= 0) & (hi <= a), 'middle': (lo >= a) & (hi <= a + mid), 'last': (lo >= a + mid) & (hi <= int(n_out[0]))}
    assert all(p.sum() >= 5 for p in parts.values())
    for name, want in (('first', 1.0), ('middle', 2.0 ** (4.0 / 12.0)), ('last', 1.0)):
        got = median(f0[parts[name]]) / before
        print('{} segment: {:.3f} Hz against {:.3f} Hz, ratio off by {:.2e}'.format(name, got * before, before, abs(got / want - 1.0)))
        assert abs(got / want - 1.0) <= 1e-3
