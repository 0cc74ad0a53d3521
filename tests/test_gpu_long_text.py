"""GPU: long-text synthesis end to end on the synthetic network of eos_cases.py (B up to 6 pieces, T = 40 frames of 275 samples, 3
Griffin-Lim iterations).  ``synthesize_text`` on two texts -- three sentences of which one needs a clause cut, and a single
sentence -- is, bit for bit, the oracle's join (tests/join_oracle.py) of the pieces' ranges cut from an ``Engine.synthesize`` call
made by hand on the same packed ids with the same settings; with a loudness it is ``Engine.loudness_normalize`` of that join; the
lengths are ``join_plan``'s; a packing into calls of two rows gives the documented lengths; ``--text`` writes one file per line.

The synthetic network's spectrograms lie some 100 dB down, so the stopping threshold is taken from the pieces' own spectrogram:
below the quietest piece's loudest frame, so that every piece has an active frame."""
import numpy as np
import pytest

import eos_cases as E
import join_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 4
N_ITER = 3
MAX_CHARS = 30
KEEP_MS = 15.0          # 330 samples: two frames of 275
FADE_MS = 2.0           # 44 samples
PAUSES = {'sentence': 40.0, 'clause': 10.0, 'word': 1.0}    # paragraph and cut: the defaults
TEXTS = ['The cat sat. It saw a bird, and then it ran far away from us. Done!', 'One short line.']
PIECES = ['The cat sat.', 'It saw a bird,', 'and then it ran far away from', 'us.', 'Done!', 'One short line.']
BREAKS = ['sentence', 'clause', 'word', 'sentence', 'paragraph', 'paragraph']
PIECE_TEXT = [0, 0, 0, 0, 0, 1]
SR = 22050


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(object):
    def __init__(self):
        M, P = pkg('tacotron.model'), pkg('tacotron.params')
        self.I = pkg('tacotron.inference')
        self.case = E.E2E
        self.hp = E.hparams_of(self.case)
        self.engine = pkg().Engine(self.hp)
        self.engine.load_weights(E.weights_of(self.case))
        self.model = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.PREDICT, hparams=self.hp, engine=self.engine)
        self.dataset = pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)
        loader = P.dataset_params.dataset_loader
        assert (loader.mel_mag_ref_db, loader.mel_mag_max_db, self.hp.magnitude_power) == (E.REF_DB, E.MAX_DB, E.POWER)
        self.S, self.hop, self.win = self.case['S'], self.case['hop'], self.case['win']
        self.keep = 2
        self.pauses = self.I.pause_samples(PAUSES, SR)
        self.fade = self.I.fade_samples(FADE_MS, SR)
        assert (self.pauses['sentence'], self.pauses['clause'], self.pauses['word'], self.pauses['paragraph'], self.fade) == (882, 220, 22, 15434, 44)
        calls, piece_text, piece_break, pieces = self.I.pack_pieces(TEXTS, self.dataset, 64, MAX_CHARS)
        assert (pieces, piece_break, piece_text) == (PIECES, BREAKS, PIECE_TEXT) and len(calls) == 1
        # the threshold: below the loudest frame of the quietest piece, off every frame's maximum
        lin = self.by_hand(calls[0][1], SEED, stop=None)['linear'].to_host()
        mx = np.clip(lin.astype(np.float64), 0.0, 1.0).max(axis=2)
        values = np.unique(mx)
        top = mx.max(axis=1).min()
        below = values[values < top - 2.2 * E.OFF_THRESHOLD]
        assert len(below), 'no frame lies clearly below the quietest piece\'s loudest one'
        self.threshold_db = float(np.float32(((below[-1] + top) / 2.0 - 1.0) * E.RANGE_DB + E.REF_DB))
        self.settings = dict(stop_at_silence_db=self.threshold_db, silence_keep_ms=KEEP_MS)

    def by_hand(self, ids, seed, stop='own', power=None):
        eng = self.engine
        stop = (self.threshold_db, self.keep) if stop == 'own' else stop
        return eng.synthesize(ids, self.S, E.REF_DB, E.MAX_DB, E.POWER if power is None else power, N_ITER, self.win, self.hop, seed=seed,
                              peak_normalize=False, want_linear=True, momentum=0.0, stop_at_silence=stop, speaking_rate=1.0, pitch=0.0,
                              phase_init='random', loudness=None, alignment_stats=None)

    def expected(self, batch_size, power=None, lead_trim=True):
        """per call what the documentation says it joins: ``[(waveforms (B, N), pieces, groups, texts, tail, orphans)]`` from a call
        made by hand, the oracle's interval on its spectrogram and the formulas of ``synthesize_text``"""
        calls, piece_text, piece_break, _p = self.I.pack_pieces(TEXTS, self.dataset, batch_size, MAX_CHARS)
        thr = self.engine.speech_threshold(self.threshold_db, E.REF_DB, E.MAX_DB)
        out = []
        for k, (p0, ids) in enumerate(calls):
            res = self.by_hand(ids, SEED + k, power=power)
            lin = res['linear'].to_host()
            first_active, last_active = O.speech_interval_batch(lin, thr)
            got = self.engine.speech_interval(res['linear'], thr)
            assert got[0].to_host().tolist() == first_active.tolist() and got[1].to_host().tolist() == last_active.tolist()
            pieces, groups, texts, tail, orphans = [], [], [], [], []
            for b in range(len(ids)):
                t, gap = piece_text[p0 + b], self.pauses[piece_break[p0 + b]]
                lead = max(0, max(0, int(first_active[b]) - 1) - self.keep) if lead_trim else 0
                first = self.hop * lead
                count = self.hop * (int(res['n_frames'][b]) - 1) - first
                if first_active[b] < 0 or count < 1:
                    if texts and texts[-1] == t:
                        pieces[-1][3] += gap
                        tail[-1] += gap
                    else:
                        orphans.append((t, gap))        # (its pause goes behind what an earlier call said of the text)
                    continue
                if not texts or texts[-1] != t:
                    texts.append(t)
                    tail.append(0)
                pieces.append([b, first, count, gap])
                groups.append(len(texts) - 1)
                tail[-1] = gap
            out.append((res['wav'].to_host(), [tuple(q) for q in pieces], groups, texts, tail, orphans))
        return out

    def parts(self, calls):
        """per text the documented layout: ``[(offset, the oracle's join of the part)]`` and the text's length -- the groups of the
        calls one behind the other, between two parts of a text the pause behind the earlier one (and of the silent pieces that
        follow it) as zeros"""
        parts, total, tails = [[] for _ in TEXTS], [0] * len(TEXTS), [0] * len(TEXTS)
        for wav, pieces, groups, texts, tail, orphans in calls:
            for t, gap in orphans:
                if parts[t]:
                    tails[t] += gap
            if not pieces:
                continue
            n_out = self.engine.join_plan(wav.shape, pieces, groups, self.fade).tolist()
            want, n_oracle = O.join(wav, pieces, groups, self.fade, max(n_out))
            assert n_oracle == n_out
            for g, (t, gap) in enumerate(zip(texts, tail)):
                if parts[t]:
                    total[t] += tails[t]
                parts[t].append((total[t], want[g, :n_out[g]]))
                total[t] += n_out[g]
                tails[t] = gap
        return parts, total

    def lengths(self, calls):
        return self.parts(calls)[1]


@pytest.fixture(scope='module')
def case():
    c = Case()
    yield c
    c.engine.close()


def run(c, **kw):
    return c.I.synthesize_text(c.model, TEXTS, c.dataset, pauses_ms=PAUSES, fade_ms=FADE_MS, max_chars=MAX_CHARS, n_steps=c.S, n_iter=N_ITER,
                               seed=SEED, **dict(c.settings, **kw))


def test_a_text_is_the_join_of_its_pieces(case):
    c = case
    (wav, pieces, groups, texts, tail, orphans), = c.expected(64)
    assert texts == [0, 1] and len(pieces) == 6 and groups == [0, 0, 0, 0, 0, 1] and not orphans   # every piece speaks
    assert any(q[1] > 0 for q in pieces) and len(set(q[2] for q in pieces)) > 1, pieces    # leads are cut, the lengths differ
    n_out = O.plan(pieces, groups, c.fade)[1]
    want, _n = O.join(wav, pieces, groups, c.fade, max(n_out))
    got = run(c)
    assert [len(w) for w in got] == n_out == c.engine.join_plan(wav.shape, pieces, groups, c.fade).tolist() == c.lengths([(wav, pieces, groups, texts, tail, orphans)])
    for g, w in enumerate(got):
        assert w.dtype == np.float32 and np.array_equal(bits(w), bits(want[g, :n_out[g]])), g
    # the pauses are zeros, and the text is not one piece
    o = O.plan(pieces, groups, c.fade)[0]
    assert not got[0][o[0] + pieces[0][2]:o[1]].any() and o[1] - o[0] - pieces[0][2] == 882
    # without the lead trim every piece starts at its row's start
    (wav0, pieces0, groups0, _t, _l, _o), = c.expected(64, lead_trim=False)
    assert all(q[1] == 0 for q in pieces0) and np.array_equal(bits(wav0), bits(wav))
    want0, _n = O.join(wav0, pieces0, groups0, c.fade, max(O.plan(pieces0, groups0, c.fade)[1]))
    got0 = run(c, lead_trim=False)
    assert all(np.array_equal(bits(w), bits(want0[g, :len(w)])) for g, w in enumerate(got0)) and len(got0[0]) > len(got[0])
    # with the attention diagnostics: the same waveforms, one record per piece
    wavs, records, verdicts, piece_text = run(c, check_alignment=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(wavs, got))
    assert len(records) == len(verdicts) == 6 and piece_text == PIECE_TEXT and records['n_sent'].tolist() == [len(p.replace('.', '')) + 1 for p in PIECES]


def test_with_a_loudness_the_joined_text_is_levelled_as_a_whole(case):
    """at a power of 0.3 (the synthetic network's waveforms lie below the -70 LUFS gate at the reference's 1.3) and measured at
    8 kHz, where the joined rows hold several blocks"""
    c = case
    target = (-23.0, 1e6)
    c.hp.magnitude_power, c.engine.sampling_rate = 0.3, 8000
    try:
        (wav, pieces, groups, _texts, _tail, _orphans), = c.expected(64, power=0.3)
        n_out = O.plan(pieces, groups, c.fade)[1]
        joined, _n = O.join(wav, pieces, groups, c.fade, -(-max(n_out) // 4) * 4)
        plain = run(c)
        assert all(np.array_equal(bits(w), bits(joined[g, :n_out[g]])) for g, w in enumerate(plain))
        want, gains = c.engine.loudness_normalize(c.engine.to_device(joined), 8000, target[0], target[1], n_samples=np.array(n_out))
        want = want.to_host()
        assert np.all(np.isfinite(gains)) and gains[0] != 1.0, gains      # (the five pieces of the first text are several blocks)
        got = run(c, loudness=target)
        assert [len(w) for w in got] == n_out
        assert all(np.array_equal(bits(w), bits(want[g, :n_out[g]])) for g, w in enumerate(got))
        # one gain per text: the sentences keep their relative levels
        for g, w in enumerate(got):
            said = np.abs(plain[g]) > 1e-20
            assert said.any() and np.allclose(w[said] / plain[g][said], gains[g], rtol=1e-6, atol=0)
    finally:
        c.hp.magnitude_power, c.engine.sampling_rate = E.POWER, SR


def test_a_packing_into_calls_of_two_rows_gives_the_documented_lengths(case):
    """every part of a text is the oracle's join of its call, bit for bit, at the documented offset, with zeros between the parts"""
    c = case
    calls = c.expected(2)
    assert len(calls) == 3
    parts, want = c.parts(calls)
    assert len(parts[0]) >= 2, 'the first text is said by one call only'      # (it spans three calls of two rows)
    got = run(c, batch_size=2)
    assert [len(w) for w in got] == want
    for t, w in enumerate(got):
        covered = np.zeros(len(w), bool)
        for offset, part in parts[t]:
            assert np.array_equal(bits(w[offset:offset + len(part)]), bits(part)), (t, offset)
            covered[offset:offset + len(part)] = True
        assert not w[~covered].view(np.uint32).any()                          # the pauses between the parts are +0.0


def test_the_command_line_writes_one_file_per_text(case, tmp_path, monkeypatch):
    c = case
    P, io = pkg('tacotron.params'), pkg('audio.io')
    lines = ['The cat sat. It ran.\\n\\nDone!', 'One short line.']
    (tmp_path / 'texts.txt').write_text('\n'.join(lines) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    np.savez(tmp_path / 'weights.npz', **E.weights_of(E.E2E))
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', c.S * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    assert c.I.main(['--synthesis-file', str(tmp_path / 'texts.txt'), '--synthesis-dir', str(out), '--weights', str(tmp_path / 'weights.npz'),
                     '--text', '--stop-at-silence', repr(c.threshold_db), '--silence-keep-ms', '0', '--pause-ms', 'sentence=40',
                     '--pause-ms', 'paragraph=100', '--fade-ms', '2', '--max-chars', '40']) == 0
    assert sorted(p.name for p in out.iterdir()) == ['1.wav', '2.wav']
    # what the files must hold: synthesize_text on the same lines with the same settings, peak-normalised once
    want = c.I.synthesize_text(c.model, c.I.read_texts(str(tmp_path / 'texts.txt')), c.dataset, pauses_ms={'sentence': 40.0, 'paragraph': 100.0},
                               fade_ms=2.0, max_chars=40, n_steps=c.S, n_iter=2, seed=0, stop_at_silence_db=c.threshold_db, silence_keep_ms=0.0)
    assert len(want) == 2 and sum(len(w) for w in want) > 0
    for i, w in enumerate(want):
        wav, sr = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert sr == SR and len(wav) == len(w), (i, len(wav), len(w))
        if len(w):
            assert np.isfinite(wav).all() and abs(np.abs(wav).max() - 1.0) < 1e-6          # peak-normalised once, by save_wav
            assert np.allclose(wav, w / np.abs(w).max(), rtol=1e-5, atol=1e-7)
