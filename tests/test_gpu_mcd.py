"""GPU: mel-cepstral distortion end to end -- tacotron.evaluate with ``mcd`` on the small fixture sentences
(tests/golden/network_small.npz) against the numpy oracles (tests/cepstrum_oracle.py, tests/dtw_oracle.py) applied to the very
mel rows the evaluation's own ``evaluate_device`` calls returned, with and without ``mcd_stop_at_silence``; what stays as it was
with ``mcd`` off; and a batch against itself."""
import json
import os

import numpy as np
import pytest

import cepstrum_oracle as C
from conftest import pkg

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
MEL_DB = (6.02, 99.89)
LIN_DB = (35.66, 100.0)


@pytest.fixture(scope='module')
def model(hparams, weights):
    M = pkg('tacotron.model')
    m = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.EVAL, weights=weights, hparams=hparams)
    m.restore = lambda checkpoint_file: None      # (the weights are loaded; restoring a checkpoint is tests/test_gpu_evaluate.py's)
    m.calls = []
    device = m.evaluate_device

    def recording(sentences, mel_specs, lin_specs, **kw):
        out = device(sentences, mel_specs, lin_specs, **kw)
        m.calls.append({k: (v.to_host().copy() if hasattr(v, 'to_host') else v) for k, v in out.items() if v is not None})
        return out

    m.evaluate_device = recording
    yield m
    m.engine.close()


def _batches(hp):
    """two small feed dicts: the fixture's two sentences, and three more; normalised-dB-like targets with zero padding"""
    g = np.load(os.path.join(GOLD, 'network_small.npz'))
    rng = np.random.default_rng(11)
    r, F = hp.reduction, 1 + hp.n_fft // 2
    feeds = []
    for ids, steps in ((g['ids'], [4, 3]), (rng.integers(2, 39, (3, 9)).astype(np.int32), [2, 5, 4])):
        B, S = ids.shape[0], max(steps)
        mel = np.zeros((B, S, r * hp.n_mels), np.float32)
        lin = np.zeros((B, S, r * F), np.float32)
        for b, s in enumerate(steps):
            mel[b, :s] = 0.5 + 0.4 * np.sin(np.cumsum(rng.standard_normal((s, r * hp.n_mels)) * 0.3, axis=1)).astype(np.float32)
            lin[b, :s] = rng.random((s, r * F)).astype(np.float32)
        feeds.append({'ph_sentences': ids, 'ph_sentence_length': np.full(B, ids.shape[1], np.int32), 'ph_mel_specs': mel,
                      'ph_lin_specs': lin, 'ph_time_frames': np.asarray(steps, np.int32)})
    return feeds


def _oracle_mcd(feeds, calls, hp, n_pred=None):
    r = hp.reduction
    per = []
    for k, (feed, call) in enumerate(zip(feeds, calls)):
        B = feed['ph_sentences'].shape[0]
        n_t = feed['ph_time_frames'].astype(np.int64) * r
        n_p = n_t if n_pred is None else n_pred[k]
        target = feed['ph_mel_specs'].reshape(B, -1, hp.n_mels)
        per.append(C.mel_cepstral_distortion(call['mel'], target, n_p, n_t, 13, *MEL_DB)[0])
    return np.concatenate(per)


def test_evaluate_with_mcd_equals_the_oracle(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    del model.calls[:]
    res = E.evaluate(model, 'model.ckpt-77', feeds, checkpoint_dir=str(tmp_path), mcd=True, verbose=False)
    assert len(model.calls) == 2 and all('mel' in c and 'linear' not in c for c in model.calls)
    per = _oracle_mcd(feeds, model.calls, hparams)
    print('mcd {:.9f} dB, oracle {:.9f} dB over {} utterances: {}'.format(res['mcd'], per.mean(), per.size, per))
    assert res['mcd_utterances'] == 5 and np.isfinite(per).all() and per.min() > 0
    assert abs(res['mcd'] - per.mean()) <= 1e-12 * per.mean()
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert line['metric/mcd'] == res['mcd'] and line['loss/loss'] == res['loss']


def test_evaluate_with_mcd_and_stop_at_silence(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    # a level that cuts: the median over the frames of the FIRST batch's predicted linear rows of their largest value
    first = model.engine.evaluate(feeds[0]['ph_sentences'], feeds[0]['ph_mel_specs'], feeds[0]['ph_lin_specs'], want_linear=True)
    top = np.sort(first['linear'].to_host().max(axis=2).reshape(-1))
    x = 0.5 * (float(top[top.size // 2 - 1]) + float(top[top.size // 2]))
    level_db = (x - 1.0) * (abs(LIN_DB[0]) + abs(LIN_DB[1])) + LIN_DB[0]
    del model.calls[:]
    res = E.evaluate(model, 'model.ckpt-78', feeds, checkpoint_dir=str(tmp_path), mcd=True, mcd_stop_at_silence=level_db, verbose=False)
    assert len(model.calls) == 2 and all('mel' in c and 'linear' in c for c in model.calls)
    thr = model.engine.speech_threshold(level_db, *LIN_DB)
    n_pred = []
    for c in model.calls:
        active = c['linear'].max(axis=2) > thr                                   # (B, T)
        last = np.where(active.any(axis=1), active.shape[1] - 1 - np.argmax(active[:, ::-1], axis=1), -1)
        n_pred.append(np.maximum(1, last + 1))
    r = hparams.reduction
    assert any((n != f['ph_time_frames'] * r).any() for n, f in zip(n_pred, feeds)), 'the level cuts nothing'
    per = _oracle_mcd(feeds, model.calls, hparams, n_pred)
    print('mcd {:.9f} dB, oracle {:.9f} dB; predicted frames {}'.format(res['mcd'], per.mean(), [n.tolist() for n in n_pred]))
    assert abs(res['mcd'] - per.mean()) <= 1e-12 * per.mean()


def test_without_mcd_the_result_and_the_line_are_the_parents(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    del model.calls[:]
    res = E.evaluate(model, 'model.ckpt-79', feeds, checkpoint_dir=str(tmp_path), verbose=False)
    assert sorted(res) == ['global_step', 'loss', 'loss_decoder', 'loss_post_processing', 'n_batches']
    assert all(sorted(c) == ['losses', 'n_steps'] for c in model.calls)      # no mel, no linear was asked for
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert sorted(line) == ['checkpoint', 'global_step', 'loss/loss', 'loss/loss_decoder', 'loss/loss_post_processing', 'n_batches']
    with_mcd = E.evaluate(model, 'model.ckpt-79', feeds, checkpoint_dir=None, mcd=True, verbose=False)
    assert all(with_mcd[k] == res[k] for k in res)


def test_a_batch_against_itself(engine):
    M = pkg('audio.metrics')
    rng = np.random.default_rng(12)
    mel = rng.random((3, 40, 80)).astype(np.float32)
    n = np.array([40, 17, 1], np.int32)
    out = M.mel_cepstral_distortion(mel, mel.copy(), n_a=n, n_b=n, engine=engine, want_path=True)
    assert (out['mcd'] == 0.0).all() and (out['cost'] == 0.0).all() and np.array_equal(out['path_len'], n)
    for b in range(3):
        assert np.array_equal(out['path'][b, :n[b], 0], np.arange(n[b])) and np.array_equal(out['path'][b, :n[b], 1], np.arange(n[b]))
        assert (out['path'][b, n[b]:] == -1).all()
    # ... and against another batch: the oracle's figure, from the oracle's own cepstra
    other = rng.random((3, 33, 80)).astype(np.float32)
    m = np.array([33, 20, 5], np.int32)
    got = M.mel_cepstral_distortion(mel, other, n_a=n, n_b=m, engine=engine)
    ref = C.mel_cepstral_distortion(mel, other, n, m, 13, *MEL_DB)
    assert np.array_equal(got['path_len'], ref[2]) and np.all(np.abs(got['mcd'] - ref[0]) <= 1e-12 * ref[0])
