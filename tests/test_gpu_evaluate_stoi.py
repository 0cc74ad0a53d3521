"""GPU: tacotron.evaluate with ``stoi`` on the small fixture sentences (tests/golden/network_small.npz): the keys appear, the
figure equals the numpy oracle (tests/stoi_oracle.py) on the waveforms the run itself made -- brought to 10 kHz by the engine's
own resampler -- and with ``stoi`` off the result and the summary line are the parent's, key for key."""
import json
import os

import numpy as np
import pytest

import stoi_oracle as S
from conftest import pkg

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
STEPS = 24      # decoder steps of the longest utterance: 120 frames of 275 samples, 1.5 s -- room for a few segments at 10 kHz


@pytest.fixture(scope='module')
def model(hparams, weights):
    M = pkg('tacotron.model')
    m = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.EVAL, weights=weights, hparams=hparams)
    m.restore = lambda checkpoint_file: None      # (the weights are loaded; restoring a checkpoint is tests/test_gpu_evaluate.py's)
    yield m
    m.engine.close()


def _batches(hp):
    """two small feed dicts: the fixture's two sentences, and three more; smooth normalised-dB-like targets with zero padding"""
    g = np.load(os.path.join(GOLD, 'network_small.npz'))
    rng = np.random.default_rng(11)
    r, F = hp.reduction, 1 + hp.n_fft // 2
    feeds = []
    for ids, steps in ((g['ids'], [STEPS, STEPS - 3]), (rng.integers(2, 39, (3, 9)).astype(np.int32), [2, STEPS, STEPS - 1])):
        B, Smax = ids.shape[0], max(steps)
        mel = np.zeros((B, Smax, r * hp.n_mels), np.float32)
        lin = np.zeros((B, Smax, r * F), np.float32)
        for b, s in enumerate(steps):
            mel[b, :s] = 0.5 + 0.4 * np.sin(np.cumsum(rng.standard_normal((s, r * hp.n_mels)) * 0.3, axis=1)).astype(np.float32)
            # a spectrum that falls with the frequency and moves with the time
            t = np.arange(s * r)[:, None]
            f = np.arange(F)[None, :]
            rows = 0.75 - 0.5 * f / F + 0.2 * np.sin(2 * np.pi * (t / 9.0 + f / 40.0)) + 0.05 * rng.standard_normal((s * r, F))
            lin[b, :s] = np.clip(rows, 0.0, 1.0).astype(np.float32).reshape(s, r * F)
        feeds.append({'ph_sentences': ids, 'ph_sentence_length': np.full(B, ids.shape[1], np.int32), 'ph_mel_specs': mel,
                      'ph_lin_specs': lin, 'ph_time_frames': np.asarray(steps, np.int32)})
    return feeds


@pytest.mark.parametrize('estoi', [False, True])
def test_evaluate_with_stoi(model, hparams, tmp_path, estoi):
    E, H = pkg('tacotron.evaluate'), pkg('_hip')
    feeds = _batches(hparams)
    key = 'metric/estoi' if estoi else 'metric/stoi'
    res = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=str(tmp_path), stoi=True, estoi=estoi, stoi_iters=3, verbose=False)
    assert sorted(res) == sorted(['global_step', 'loss', 'loss_decoder', 'loss_post_processing', 'n_batches', 'stoi_utterances', key])
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert line[key] == res[key] and line['stoi_utterances'] == res['stoi_utterances']
    assert ('metric/stoi' if estoi else 'metric/estoi') not in line
    # the same chain by hand: the waveforms the run made, the engine's resampler, the oracle
    eng = model.engine
    ratio = 10000.0 / hparams.sampling_rate
    finite, bound = [], 0.0
    for feed in feeds:
        values, ref, deg, lens = E.batch_stoi(model, feed, extended=estoi, stoi_iters=3, want_wavs=True)
        for b, n in enumerate(lens):
            r10, d10 = eng.resample(ref[b, :n], ratio), eng.resample(deg[b, :n], ratio)
            valid = H.resampled_valid(int(n), ratio)
            o = S.stoi(r10.to_host()[:valid], d10.to_host()[:valid], estoi)
            r10.free()
            d10.free()
            assert np.isnan(values[b]) == np.isnan(o['value']), (b, values[b], o['value'])
            if np.isfinite(o['value']):
                assert o['degenerate'] == 0
                assert abs(values[b] - o['value']) <= S.value_bound(o, estoi), (b, values[b], o['value'])
                bound = max(bound, S.value_bound(o, estoi))
                finite.append(values[b])
    assert res['stoi_utterances'] == len(finite) == 4              # the utterance of two decoder steps is too short for a segment
    assert abs(res[key] - float(np.mean(finite))) <= 1e-15
    # together with the distortion: its figure is the one mcd alone reports
    both = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=None, mcd=True, stoi=True, estoi=estoi, stoi_iters=3, verbose=False)
    alone = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=None, mcd=True, verbose=False)
    assert both['mcd'] == alone['mcd'] and both[key] == res[key]


def test_without_stoi_the_result_is_the_parents(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    res = E.evaluate(model, 'model.ckpt-81', feeds, checkpoint_dir=str(tmp_path), stoi=False, verbose=False)
    assert sorted(res) == ['global_step', 'loss', 'loss_decoder', 'loss_post_processing', 'n_batches']
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert sorted(line) == ['checkpoint', 'global_step', 'loss/loss', 'loss/loss_decoder', 'loss/loss_post_processing', 'n_batches']
    with_stoi = E.evaluate(model, 'model.ckpt-81', feeds, checkpoint_dir=None, stoi=True, stoi_iters=2, verbose=False)
    assert all(with_stoi[k] == res[k] for k in res)
