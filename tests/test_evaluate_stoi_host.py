"""tacotron.evaluate and its ``stoi`` switch without a GPU: with ``stoi`` off the run asks the model for what it always asked --
and never for a teacher-forced pass --, and the result, the printed lines and the summary line are what they always were;
``--estoi`` and ``--stoi-iters`` need ``--stoi``.  tacotron.dataset_statistics: ``--estoi`` needs ``--reconstruction-stoi``."""
import inspect
import json

import numpy as np
import pytest

from conftest import pkg


class _Losses(object):
    def __init__(self, values):
        self.values = np.asarray(values, np.float32)

    def to_host(self):
        return self.values


class _Model(object):
    """a Tacotron in Mode.EVAL as far as evaluate() looks: it records what every batch was asked for"""

    def __init__(self):
        self._mode = pkg('tacotron.model').Mode.EVAL
        self.asked = []
        self.forced = []

    def restore(self, checkpoint_file):
        pass

    def evaluate_device(self, sentences, mel_specs, lin_specs, **kw):
        self.asked.append(kw)
        k = len(self.asked)
        return {'losses': _Losses([0.5 * k, 0.25 * k, 0.125 * k]), 'n_steps': 3}

    def teacher_forced_device(self, sentences, mel_specs, lin_specs=None, **kw):
        self.forced.append((lin_specs, kw))
        raise RuntimeError('no engine to go on with')


def _feeds():
    return [{'ph_sentences': np.zeros((2, 5), np.int32), 'ph_mel_specs': None, 'ph_lin_specs': None} for _ in range(3)]


def test_without_stoi_the_run_the_result_and_the_lines_are_the_parents(tmp_path, capsys):
    E = pkg('tacotron.evaluate')
    for fn in (E.evaluate, E.evaluate_checkpoint):
        sig = inspect.signature(fn)
        assert sig.parameters['stoi'].default is False and sig.parameters['estoi'].default is False
        assert sig.parameters['stoi_iters'].default is None
    results = []
    for kw in ({}, {'stoi': False}):
        m = _Model()
        results.append(E.evaluate(m, 'run/model.ckpt-1234', _feeds(), checkpoint_dir=str(tmp_path), checkpoint_save_run='ev', **kw))
        assert m.asked == [dict(want_mel=False, want_alignments=False, want_linear=False)] * 3 and m.forced == []
    want = dict(loss=1.0, loss_decoder=0.5, loss_post_processing=0.25, global_step=1234, n_batches=3)
    assert results[0] == want and results[1] == want
    printed = capsys.readouterr().out.splitlines()
    assert printed.count('[evaluate] step: 1234, batches: 3, loss: 1.000000, loss_decoder: 0.500000, loss_post_processing: 0.250000') == 2
    assert not any('stoi' in line for line in printed)
    with open(str(tmp_path / 'ev' / E.SUMMARY_FILE)) as f:
        lines = [json.loads(line) for line in f]
    assert len(lines) == 2 and lines[0] == lines[1] == {
        'global_step': 1234, 'checkpoint': 'run/model.ckpt-1234', 'n_batches': 3, 'loss/loss': 1.0, 'loss/loss_decoder': 0.5,
        'loss/loss_post_processing': 0.25}


def test_stoi_makes_one_teacher_forced_call_per_batch_with_want_linear():
    E = pkg('tacotron.evaluate')
    P = pkg('tacotron.params')

    class _WithParams(_Model):
        hparams = P.ModelParams()
        engine = type('E', (), {'cfg': type('C', (), {'reduction': P.ModelParams().reduction})()})()

    m = _WithParams()
    F = 1 + m.hparams.n_fft // 2
    feed = {'ph_sentences': np.zeros((2, 5), np.int32), 'ph_mel_specs': np.zeros((2, 4, m.hparams.reduction * m.hparams.n_mels), np.float32),
            'ph_lin_specs': np.zeros((2, 4, m.hparams.reduction * F), np.float32), 'ph_time_frames': np.array([4, 3], np.int32)}
    with pytest.raises(RuntimeError):      # (this model has no engine to go on with: the batch gets as far as the request)
        E.evaluate(m, 'model.ckpt-1', [feed], checkpoint_dir=None, stoi=True, verbose=False)
    assert m.asked == [dict(want_mel=False, want_alignments=False, want_linear=False)]      # the evaluation pass itself is unchanged
    assert len(m.forced) == 1 and m.forced[0] == (None, dict(want_mel=False, want_alignments=False, want_linear=True))
    with pytest.raises(ValueError):
        E.evaluate(_Model(), 'model.ckpt-1', [feed], checkpoint_dir=None, estoi=True, verbose=False)


@pytest.mark.parametrize('argv', [['--estoi'], ['--stoi-iters', '10'], ['--mcd', '--estoi'], ['--stoi', '--stoi-iters', '-1'],
                                  ['--stoi', '--stoi-iters', 'many']])
def test_option_errors(argv, capsys):
    E = pkg('tacotron.evaluate')
    with pytest.raises(SystemExit) as e:
        E.main(argv + ['--checkpoint-dir', '/nonexistent'])
    assert e.value.code == 2
    assert 'stoi' in capsys.readouterr().err


def test_legal_options_get_as_far_as_the_checkpoint_listing():
    E = pkg('tacotron.evaluate')
    for argv in (['--stoi'], ['--stoi', '--estoi'], ['--stoi', '--stoi-iters', '10'], ['--mcd', '--f0', '--stoi', '--estoi']):
        with pytest.raises(FileNotFoundError):
            E.main(argv + ['--checkpoint-dir', '/nonexistent'])


@pytest.mark.parametrize('argv', [['--estoi'], ['--reconstruction-stoi', '0'], ['--reconstruction-stoi', 'many']])
def test_dataset_statistics_option_errors(argv, capsys):
    D = pkg('tacotron.dataset_statistics')
    with pytest.raises(SystemExit) as e:
        D.main(argv + ['--dataset-folder', '/nonexistent'])
    assert e.value.code == 2
    assert 'stoi' in capsys.readouterr().err
