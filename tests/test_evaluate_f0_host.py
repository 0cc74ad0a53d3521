"""tacotron.evaluate and its ``f0`` switch without a GPU: with ``f0`` off the run asks the model for what it always asked, and the
result, the printed lines and the summary line are what they always were; the ``--f0-*`` options need ``--f0`` and refuse values
that make no search range."""
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
        self.restored = []

    def restore(self, checkpoint_file):
        self.restored.append(checkpoint_file)

    def evaluate_device(self, sentences, mel_specs, lin_specs, **kw):
        self.asked.append(kw)
        k = len(self.asked)
        return {'losses': _Losses([0.5 * k, 0.25 * k, 0.125 * k]), 'n_steps': 3}


def _feeds():
    return [{'ph_sentences': np.zeros((2, 5), np.int32), 'ph_mel_specs': None, 'ph_lin_specs': None} for _ in range(3)]


def test_without_f0_the_run_the_result_and_the_lines_are_the_parents(tmp_path, capsys):
    E = pkg('tacotron.evaluate')
    sig = inspect.signature(E.evaluate)
    assert sig.parameters['f0'].default is False and sig.parameters['f0_iters'].default is None
    assert sig.parameters['f0_min'].default == 60.0 and sig.parameters['f0_max'].default == 500.0
    sig = inspect.signature(E.evaluate_checkpoint)
    assert sig.parameters['f0'].default is False and sig.parameters['f0_iters'].default is None
    results = []
    for kw in ({}, {'f0': False}):
        m = _Model()
        results.append(E.evaluate(m, 'run/model.ckpt-1234', _feeds(), checkpoint_dir=str(tmp_path), checkpoint_save_run='ev', **kw))
        assert m.restored == ['run/model.ckpt-1234']
        assert m.asked == [dict(want_mel=False, want_alignments=False, want_linear=False)] * 3
    want = dict(loss=1.0, loss_decoder=0.5, loss_post_processing=0.25, global_step=1234, n_batches=3)
    assert results[0] == want and results[1] == want
    printed = capsys.readouterr().out.splitlines()
    assert printed.count('[evaluate] step: 1234, batches: 3, loss: 1.000000, loss_decoder: 0.500000, loss_post_processing: 0.250000') == 2
    assert not any('f0' in line or 'mcd' in line for line in printed)
    with open(str(tmp_path / 'ev' / E.SUMMARY_FILE)) as f:
        lines = [json.loads(line) for line in f]
    assert len(lines) == 2 and lines[0] == lines[1] == {
        'global_step': 1234, 'checkpoint': 'run/model.ckpt-1234', 'n_batches': 3, 'loss/loss': 1.0, 'loss/loss_decoder': 0.5,
        'loss/loss_post_processing': 0.25}


def test_f0_asks_every_batch_for_its_mel_and_linear_rows():
    E = pkg('tacotron.evaluate')
    m = _Model()
    with pytest.raises(Exception):      # (this model has no engine to measure with: the first batch gets as far as the request)
        E.evaluate(m, 'model.ckpt-1', _feeds(), checkpoint_dir=None, f0=True, verbose=False)
    assert m.asked == [dict(want_mel=True, want_alignments=False, want_linear=True)]
    assert E.F0_KEYS == ('f0_rmse_cents', 'f0_rmse_hz', 'vuv_error', 'gross_pitch_error')


@pytest.mark.parametrize('argv', [['--f0-iters', '10'], ['--f0-min', '80'], ['--f0-max', '400'], ['--mcd', '--f0-min', '80'],
                                  ['--f0', '--f0-min', '400', '--f0-max', '80'], ['--f0', '--f0-min', '0'], ['--f0', '--f0-iters', '-1'],
                                  ['--f0', '--f0-iters', 'many']])
def test_option_errors(argv, capsys):
    E = pkg('tacotron.evaluate')
    with pytest.raises(SystemExit) as e:
        E.main(argv + ['--checkpoint-dir', '/nonexistent'])
    assert e.value.code == 2
    assert 'f0' in capsys.readouterr().err


def test_legal_options_get_as_far_as_the_checkpoint_listing():
    E = pkg('tacotron.evaluate')
    for argv in (['--f0'], ['--f0', '--f0-iters', '10', '--f0-min', '80', '--f0-max', '400'], ['--mcd', '--f0', '--mcd-coeffs', '5']):
        with pytest.raises(FileNotFoundError):
            E.main(argv + ['--checkpoint-dir', '/nonexistent'])
