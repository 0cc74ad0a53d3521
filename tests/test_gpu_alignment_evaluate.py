"""GPU: ``tacotron.evaluate --attention``.  The per-checkpoint counts of every flag and the mean focus equal what the numpy oracle
of tests/alignment_oracle.py and ``attention_check.verdict`` make of each batch's alignments -- fetched from the engine by hand,
with the batch's own sentence lengths and frame counts -- and without the switch nothing of the result or the summary line
changes."""
import json
import os

import numpy as np
import pytest

import alignment_oracle as O
from conftest import pkg
from tf_bundle_writer import write_tensor_bundle

pytestmark = pytest.mark.gpu


def _dataset(root, hp, n=20):
    rng = np.random.default_rng(31)
    words = ['a', 'cat', 'sat', 'on', 'the', 'mat', 'dog', 'ran']
    os.makedirs(os.path.join(root, 'wavs'))
    F = 1 + hp.n_fft // 2
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for i in range(n):
            text = ' '.join(rng.choice(words, 1 + i % 4))
            fid = 'LJ{:03d}'.format(i)
            f.write('{}|{}|{}\n'.format(fid, text.upper(), text))
            t_red = 1 + int(rng.integers(0, 5))
            np.savez(os.path.join(root, 'wavs', fid + '.npz'), mel_mag_db=rng.random((t_red, hp.n_mels * hp.reduction)).astype(np.float32),
                     linear_mag_db=rng.random((t_red, F * hp.reduction)).astype(np.float32))


def test_evaluate_reports_the_flags_and_the_mean_focus(engine, tmp_path, hparams, weights):
    C = pkg('tacotron.checkpoint')
    E = pkg('tacotron.evaluate')
    A = pkg('tacotron.attention_check')
    P = pkg('tacotron.params')
    data = str(tmp_path / 'data')
    _dataset(data, hparams)
    run = tmp_path / 'ckpt' / 'train'
    run.mkdir(parents=True)
    ck = dict(weights)
    ck['global_step'] = np.array(700, dtype=np.int64)
    write_tensor_bundle(str(run / 'model.ckpt-700'), ck, block_entries=16, crc_fn=C.crc32c)
    (run / 'checkpoint').write_text('model_checkpoint_path: "model.ckpt-700"\nall_model_checkpoint_paths: "model.ckpt-700"\n')
    # by hand: every batch's alignments through the oracle
    helper = pkg('datasets.lj_speech').LJSpeechDatasetHelper(data, P.dataset_params.vocabulary_dict, False)
    records = []
    for feed in E.batched_placeholders(helper, 20, 4, verbose=False):
        out = engine.evaluate(feed['ph_sentences'], feed['ph_mel_specs'], feed['ph_lin_specs'], want_mel=False, want_alignments=True,
                              want_linear=False)
        records.append(O.batch(out['alignments'].to_host(), feed['ph_sentence_length'], feed['ph_time_frames'])[0])
    every = np.concatenate(records)
    verdicts = A.verdict(every)
    kw = dict(dataset_folder=data, max_samples=20, batch_size=4, checkpoint_dir=str(tmp_path / 'ckpt'), hparams=hparams, verbose=False)
    plain = E.evaluate_checkpoint(str(run / 'model.ckpt-700'), **kw)
    res = E.evaluate_checkpoint(str(run / 'model.ckpt-700'), attention=True, **kw)
    assert not any(k.startswith('attention') for k in plain)
    assert {k: v for k, v in res.items() if not k.startswith('attention')} == plain
    assert res['attention_utterances'] == 20 == len(every)
    for flag in A.FLAGS:
        assert res['attention/' + flag] == sum(flag in v for v in verdicts), flag
    assert res['attention/mean_focus'] == float(np.mean(every['focus_sum'] / every['n_steps']))
    with open(str(tmp_path / 'ckpt' / 'evaluate' / E.SUMMARY_FILE)) as f:
        lines = [json.loads(line) for line in f]
    assert not any(k.startswith('attention') for k in lines[0])
    assert {k: v for k, v in lines[1].items() if k.startswith('attention')} == {k: v for k, v in res.items() if k.startswith('attention')}
    argv = ['--checkpoint-dir', str(tmp_path / 'ckpt'), '--dataset-folder', data, '--max-samples', '20', '--batch-size', '4', '--attention']
    assert E.main(argv) == 0
