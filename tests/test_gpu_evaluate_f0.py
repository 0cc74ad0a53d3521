"""GPU: tacotron.evaluate with ``f0`` on the small fixture sentences (tests/golden/network_small.npz): the four figures and their
counts come out finite, equal to the same chain run by hand on the evaluation's own outputs -- de-normalisation, ** power, ragged
Griffin-Lim, tts_f0, tts_f0_compare along the alignment of the distortion -- and with ``f0`` off the result is the parent's, key
for key."""
import json
import os

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def model(hparams, weights):
    M = pkg('tacotron.model')
    m = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.EVAL, weights=weights, hparams=hparams)
    m.restore = lambda checkpoint_file: None      # (the weights are loaded; restoring a checkpoint is tests/test_gpu_evaluate.py's)
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


def test_evaluate_with_f0(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    res = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=str(tmp_path), f0=True, f0_iters=5, verbose=False)
    keys = ['metric/' + k for k in E.F0_KEYS]
    assert sorted(res) == sorted(['global_step', 'loss', 'loss_decoder', 'loss_post_processing', 'n_batches', 'f0_utterances'] + keys)
    assert 0 <= res['f0_utterances'] <= 5
    assert np.isfinite(res['metric/vuv_error']) and 0.0 <= res['metric/vuv_error'] <= 1.0
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    for k in keys:
        assert (line[k] == res[k]) or (np.isnan(line[k]) and np.isnan(res[k]))
    assert line['f0_utterances'] == res['f0_utterances'] and 'metric/mcd' not in line
    # the same chain by hand, batch by batch: finite counts, and the means evaluate() reports
    per = {k: [] for k in E.F0_KEYS}
    for feed in feeds:
        out = model.evaluate_device(feed['ph_sentences'], feed['ph_mel_specs'], feed['ph_lin_specs'], want_mel=True,
                                    want_alignments=False, want_linear=True)
        align, n_pred, n_target = E.batch_alignment(model, feed, out, want_path=True)
        errs = E.batch_f0(model, feed, out, align['path'], n_pred, n_target, f0_iters=5)
        B = feed['ph_sentences'].shape[0]
        assert errs['counts'].shape == (B, 5) and (errs['counts'] >= 0).all()
        assert np.array_equal(errs['counts'][:, 0], align['path_len'])
        assert (errs['counts'][:, 1] + errs['counts'][:, 2] + errs['counts'][:, 4] <= errs['counts'][:, 0]).all()
        for k in E.F0_KEYS:
            per[k].append(errs[k])
    for k in E.F0_KEYS:
        v = np.concatenate(per[k])
        v = v[np.isfinite(v)]
        if v.size:
            assert res['metric/' + k] == float(np.mean(v)), k
        else:
            assert np.isnan(res['metric/' + k]), k
    assert res['f0_utterances'] == int(np.isfinite(np.concatenate(per['f0_rmse_cents'])).sum())
    # together with the distortion: its figure is the one mcd alone reports
    both = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=None, mcd=True, f0=True, f0_iters=5, verbose=False)
    alone = E.evaluate(model, 'model.ckpt-80', feeds, checkpoint_dir=None, mcd=True, verbose=False)
    assert both['mcd'] == alone['mcd'] and both['mcd_utterances'] == 5 and all(both[k] == res[k] or np.isnan(res[k]) for k in keys)


def test_without_f0_the_result_is_the_parents(model, hparams, tmp_path):
    E = pkg('tacotron.evaluate')
    feeds = _batches(hparams)
    res = E.evaluate(model, 'model.ckpt-81', feeds, checkpoint_dir=str(tmp_path), f0=False, verbose=False)
    assert sorted(res) == ['global_step', 'loss', 'loss_decoder', 'loss_post_processing', 'n_batches']
    with open(str(tmp_path / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert sorted(line) == ['checkpoint', 'global_step', 'loss/loss', 'loss/loss_decoder', 'loss/loss_post_processing', 'n_batches']
    with_f0 = E.evaluate(model, 'model.ckpt-81', feeds, checkpoint_dir=None, f0=True, f0_iters=2, verbose=False)
    assert all(with_f0[k] == res[k] for k in res)


def test_a_tone_through_the_vocoder_against_itself(engine, hparams):
    """audio.metrics.f0_errors of a track against itself along the diagonal: every voiced step agrees"""
    M = pkg('audio.metrics')
    import f0_cases as K
    x = np.stack([K.tone(150.0, 5500), K.tone(220.0, 5500, seed=1)])
    f0 = engine.f0(x, K.SR, 275)
    T = f0.shape[1]
    path = np.stack([K.diagonal_path(T, T, 2 * T - 1)] * 2)
    out = M.f0_errors(f0, f0, path, engine=engine)
    f0.free()
    assert (out['counts'][:, 0] == T).all() and (out['counts'][:, 1] >= T // 2).all() and (out['counts'][:, 2:] == 0).all()
    assert (out['f0_rmse_hz'] == 0).all() and (out['f0_rmse_cents'] == 0).all() and (out['vuv_error'] == 0).all()
    assert (out['gross_pitch_error'] == 0).all()
