"""GPU: the delivery format above the engine -- ``output=`` of ``tacotron.inference`` (``synthesize_batch``, ``synthesize_stream``,
``synthesize_text``), ``audio.io.save_wav(encoding=...)`` and the command line's ``--format`` / ``--out-rate`` -- on the synthetic
network and the texts of tests/test_gpu_long_text.py.  Every layer hands back the oracle's codes (tests/encode_oracle.py) of the
float32 waveforms the same helper returns without the keyword (behind ``Engine.resample`` where the rate changes)."""
import logging

import numpy as np
import pytest

import encode_cases as C
import encode_oracle as O
import eos_cases as E
import test_gpu_long_text as LT
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 6


@pytest.fixture(scope='module')
def case():
    c = LT.Case()
    yield c
    c.engine.close()


def _ids(c):
    return c.I.pack_pieces(LT.TEXTS, c.dataset, 64, LT.MAX_CHARS)[0][0][1]


def _half(engine, w, n=None):
    """row(s) at half the rate, as the host sees them"""
    r = engine.resample(w, 0.5, n_samples=n)
    out = r.to_host()
    r.free()
    return out


def test_a_batch_comes_back_in_the_format(case, caplog):
    c, ids = case, _ids(case)
    kw = dict(n_steps=c.S, n_iter=LT.N_ITER, seed=SEED, peak_normalize=True)
    w = c.I.synthesize_batch(c.model, ids, **kw)
    with caplog.at_level(logging.WARNING):
        got = c.I.synthesize_batch(c.model, ids, output='pcm16', **kw)
    want, st = O.encode(w, O.S16, O.TPDF, SEED)
    assert C.same_bits(got, want)
    # a row that reaches +1 clips, and is logged once with its count
    clipped = [b for b in range(len(ids)) if st['clipped'][b] > 0]
    assert clipped and len(caplog.records) == len(clipped)
    assert all('{} of {} samples clipped'.format(st['clipped'][b], st['n'][b]) in r.getMessage() for b, r in zip(clipped, caplog.records))
    # with stopping: every row cut to what it holds, at the output rate
    stop = dict(c.settings)
    ws = c.I.synthesize_batch(c.model, ids, **dict(kw, **stop))
    got = c.I.synthesize_batch(c.model, ids, output=('mulaw', None, 11025), **dict(kw, **stop))
    assert len(set(len(x) for x in ws)) > 1
    for b, x in enumerate(ws):
        row = _half(c.engine, x)
        assert len(got[b]) == len(row) == -(-len(x) // 2)
        assert C.same_bits(got[b], O.encode_row(row, O.MULAW, O.NONE, SEED, b)[0]), b


def test_a_stream_encodes_inside_its_calls(case):
    c, ids = case, _ids(case)
    kw = dict(n_steps=c.S, n_iter=LT.N_ITER, seed=SEED, peak_normalize=True, copy=True)
    floats = list(c.I.synthesize_stream(c.model, [ids] * 4, **kw))
    coded = list(c.I.synthesize_stream(c.model, [ids] * 4, output=('alaw', 'tpdf', None), **kw))
    assert len(coded) == 4
    for k, (w, got) in enumerate(zip(floats, coded)):
        assert C.same_bits(got, O.encode(w, O.ALAW, O.TPDF, SEED + k)[0]), k       # the dither's seed is the call's
    cut = list(c.I.synthesize_stream(c.model, [ids], output='pcm8', **dict(kw, **c.settings)))[0]
    ws = list(c.I.synthesize_stream(c.model, [ids], **dict(kw, **c.settings)))[0]
    assert [len(x) for x in cut] == [len(x) for x in ws]
    for b, x in enumerate(ws):
        assert C.same_bits(cut[b], O.encode_row(x, O.U8, O.TPDF, SEED, b)[0]), b


def test_a_text_is_encoded_as_a_whole(case):
    c = case
    plain = LT.run(c)
    peaks = [np.abs(w).max() for w in plain]
    got = LT.run(c, output=('pcm16', 'tpdf', 11025), peak_normalize=True)
    assert [g.dtype for g in got] == [np.int16, np.int16]
    for t, w in enumerate(plain):
        # the whole text normalised (a row of the batch the texts are padded to), resampled, then encoded as row t
        norm = c.engine.peak_normalize(c.engine.to_device(w[None])).to_host()[0]
        assert abs(np.abs(norm).max() - 1.0) < 1e-6 and peaks[t] > 0
        row = _half(c.engine, norm)
        assert C.same_bits(got[t], O.encode_row(row, O.S16, O.TPDF, LT.SEED, t)[0]), t
    with pytest.raises(ValueError, match='peak_normalize'):
        LT.run(c, peak_normalize=True)


def test_save_wav_encodes_on_the_device(case, tmp_path):
    c = case
    io = pkg('audio.io')
    x = np.stack([C.speech_like(2001, 0.8, seed=s) for s in (1, 2)])
    for encoding, fmt in (('pcm16', O.S16), ('pcm8', O.U8), ('mulaw', O.MULAW), ('alaw', O.ALAW)):
        for dither in (True, False):
            p = str(tmp_path / 'a.wav')
            io.save_wav(p, x[0], 8000, engine=c.engine, encoding=encoding, dither=dither)
            want = O.encode(x[:1], fmt, O.TPDF if dither else O.NONE, 0)[0][0]
            y, sr = io.load_wav(p)
            assert sr == 8000 and np.array_equal(y, O.decode(fmt, want).astype(np.float32)), (encoding, dither)
    # two channels: channel c is dithered as row c; normalised first with norm
    p = str(tmp_path / 's.wav')
    io.save_wav(p, x, 8000, True, engine=c.engine, encoding='pcm16')
    flat = c.engine.peak_normalize(c.engine.to_device(x.reshape(1, -1))).to_host().reshape(x.shape)
    want = O.encode(flat, O.S16, O.TPDF, 0)[0]
    import wave
    with wave.open(p, 'rb') as f:
        assert f.getnchannels() == 2 and np.array_equal(np.frombuffer(f.readframes(2001), '<i2').reshape(2001, 2).T, want)


def test_the_command_line_writes_the_format(case, tmp_path, monkeypatch):
    c = case
    P, io = pkg('tacotron.params'), pkg('audio.io')
    (tmp_path / 'lines.txt').write_text('The cat sat.\nOne short line.\n')
    out = tmp_path / 'out'
    out.mkdir()
    np.savez(tmp_path / 'weights.npz', **E.weights_of(E.E2E))
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', c.S * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    lines = ['The cat sat.', 'One short line.']
    common = ['--synthesis-file', str(tmp_path / 'lines.txt'), '--synthesis-dir', str(out), '--weights', str(tmp_path / 'weights.npz'), '--seed', '3']
    assert c.I.main(common + ['--format', 'mulaw', '--out-rate', '11025', '--no-dither']) == 0
    # what the files must hold: the same batch by hand, peak-normalised in the call, resampled, encoded as rows 0 and 1
    seqs, lens = c.dataset.process_sentences(lines)
    ids = np.array([c.I.pad_sentence(np.frombuffer(q, dtype=np.int32), max(lens)) for q in seqs], dtype=np.int32)
    w = c.I.synthesize_batch(c.model, ids, n_steps=c.S, n_iter=2, seed=3, peak_normalize=True)
    rows = _half(c.engine, w)
    for i in range(2):
        blob = (out / '{}.wav'.format(i + 1)).read_bytes()
        assert int.from_bytes(blob[20:22], 'little') == 7                          # WAVE_FORMAT_MULAW
        y, rate = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert rate == 11025 and len(y) == rows.shape[1]
        assert np.array_equal(y, O.decode(O.MULAW, O.encode_row(rows[i], O.MULAW, O.NONE, 3, i)[0]).astype(np.float32)), i
    # ... and without the options the files are the float32 files they always were
    assert c.I.main(common) == 0
    blob = (out / '1.wav').read_bytes()
    assert int.from_bytes(blob[20:22], 'little') == 3 and io.load_wav(str(out / '1.wav'))[1] == LT.SR


@pytest.mark.parametrize('pipelined', [False, True])
def test_serve_answers_in_the_format(weights, pipelined, monkeypatch):
    """request k, sentence b: the oracle's codes of the float32 answer, dithered with seed k as row b -- whether the call encodes
    its rows itself (pipelined) or the loop hands the reconstructed waveforms to ``deliver``"""
    S, P = pkg('tacotron.serve'), pkg('tacotron.params')
    requests = [['Hello there.', 'Hi'], ['One more.']]
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', 20)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    plain = list(S.serve(iter(requests), weights, pipelined=pipelined))
    for output, fmt, dither in (('pcm16', O.S16, O.TPDF), (('alaw', None, None), O.ALAW, O.NONE)):
        coded = list(S.serve(iter(requests), weights, pipelined=pipelined, output=output))
        assert [len(a) for a in coded] == [2, 1]
        for k, (answer, before) in enumerate(zip(coded, plain)):
            for b, (codes, w) in enumerate(zip(answer, before)):
                assert C.same_bits(np.ascontiguousarray(codes), O.encode_row(w, fmt, dither, k, b)[0]), (output, k, b)
