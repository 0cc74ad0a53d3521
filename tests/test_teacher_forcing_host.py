"""CPU: the float64 teacher-forced decoder of tests/teacher_oracle.py (reference tacotron/helpers.py:208-405,
TacotronTrainingHelper) against ``oracle.tacotron_oracle.decoder``, and the host side of the ``tacotron.gta`` entry point --
cropping, durations, file naming and the pairing of batches with their recordings -- with a stub model."""
import copy
import os

import numpy as np
import pytest

from conftest import pkg
from oracle import tacotron_oracle as O
import teacher_oracle as TO


def _config(hparams, name, cudnn):
    hp = copy.deepcopy(hparams)
    hp.force_cudnn = cudnn
    if name in ('monotonic', 'predictive'):
        hp.attention.mechanism = 'LocalLuongAttention'
        hp.attention.luong_local_window_D = 5
        hp.attention.luong_local_mode = name
    w = pkg('tacotron.weights').synthetic_weights(11, hp)
    return hp, {k: v.astype(np.float64) for k, v in w.items()}


@pytest.mark.parametrize('cudnn', [False, True], ids=['gru-cell', 'cudnn'])
@pytest.mark.parametrize('name', ['global', 'monotonic', 'predictive'])
def test_fed_the_free_run_the_restatement_reproduces_it(hparams, name, cudnn):
    """The free run feeds back the last n_mels of its own step output -- frame t*r - 1 of its mel: fed that mel as the
    target, the teacher-forced restatement is the free run."""
    hp, w = _config(hparams, name, cudnn)
    B, Ts, S = 2, 40, 7
    memory = np.random.default_rng(1).standard_normal((B, Ts, 256)) * 0.5
    ref_mel, ref_al = O.decoder(memory, w, hp, n_steps=S)
    mel, al = TO.decoder_teacher(memory, ref_mel, w, hp)
    assert np.abs(mel - ref_mel).max() <= 1e-12 * np.abs(ref_mel).max()
    assert np.abs(al - ref_al).max() <= 1e-12


def test_the_last_group_is_never_fed_and_steps_see_only_earlier_frames(hparams, weights64):
    B, Ts, S, r = 2, 15, 6, hparams.reduction
    rng = np.random.default_rng(2)
    memory = rng.standard_normal((B, Ts, 256)) * 0.5
    target = rng.random((B, S * r, hparams.n_mels))
    mel0, al0 = TO.decoder_teacher(memory, target, weights64, hparams)
    t1 = target.copy()
    t1[:, -r:] += 1.0
    mel1, al1 = TO.decoder_teacher(memory, t1, weights64, hparams)
    assert np.array_equal(mel1, mel0) and np.array_equal(al1, al0)
    for t in range(1, S):
        t2 = target.copy()
        t2[:, t * r - 1] += 1.0
        mel2, al2 = TO.decoder_teacher(memory, t2, weights64, hparams)
        assert np.array_equal(mel2[:, :t], mel0[:, :t]) and np.array_equal(al2[:t], al0[:t])
        assert not np.array_equal(mel2[:, t], mel0[:, t])
        # the other frames of a group are never read
        t3 = target.copy()
        t3[:, t * r - 2] += 1.0
        assert np.array_equal(TO.decoder_teacher(memory, t3, weights64, hparams)[0], mel0)
    x = TO.teacher_inputs(target, hparams, S)
    assert np.all(x[0] == 0) and np.array_equal(x[2], target[:, 2 * r - 1])


def test_durations_and_crop():
    G = pkg('tacotron.gta')
    al = np.zeros((4, 3), np.float32)
    al[[0, 1, 2, 3], [0, 0, 2, 1]] = 1.0
    assert G.durations(al, 5).tolist() == [10, 5, 5]
    assert G.durations(al, 5).dtype == np.int32
    r, nm, F = 2, 3, 4
    B, S, Ts = 2, 5, 6
    rng = np.random.default_rng(3)
    mel = rng.random((B, S * r, nm)).astype(np.float32)
    lin = rng.random((B, S * r, F)).astype(np.float32)
    align = rng.random((S, B, Ts)).astype(np.float32)
    out = G.crop(mel, align, lin, 1, 3, 4, r)
    assert np.array_equal(out['mel_mag_db'], mel.reshape(B, S, r * nm)[1, :3])
    assert np.array_equal(out['linear_mag_db'], lin.reshape(B, S, r * F)[1, :3])
    assert np.array_equal(out['alignments'], align[:3, 1, :4])
    # argmax over the utterance's own positions only
    assert np.array_equal(out['durations'], G.durations(align[:3, 1, :4], r))
    assert out['durations'].sum() == 3 * r
    assert 'linear_mag_db' not in G.crop(mel, align, None, 0, 5, 6, r)
    assert G.gta_path('/x/gta', '/data/wavs/LJ001-0001.wav') == os.path.join('/x/gta', 'LJ001-0001.gta.npz')


class _Dev(object):
    def __init__(self, a):
        self.a = a

    def to_host(self):
        return self.a


class _StubModel(object):
    """Echoes the targets as the predicted spectrograms; alignments from the ids, so that every file can be traced back to
    its recording and its batch row."""

    def __init__(self, hp):
        self.hparams = hp
        self.calls = []

    def teacher_forced_device(self, sentences, mel_specs, lin_specs=None, want_mel=True, want_alignments=True,
                              want_linear=True, want_sums=False):
        B, S = mel_specs.shape[:2]
        Ts = sentences.shape[1]
        self.calls.append((sentences.shape, mel_specs.shape, want_linear))
        al = np.zeros((S, B, Ts), np.float32)
        for b in range(B):
            al[:, b, :] = np.arange(Ts)[None, :] == (np.arange(S)[:, None] % Ts)
            al[:, b, -1] = 2.0   # the padding column wins wherever the batch is padded: cropped away per utterance
        nm = self.hparams.n_mels
        out = dict(mel=_Dev(mel_specs.reshape(B, -1, nm)), alignments=_Dev(al),
                   losses=_Dev(np.array([3.0, 1.0, 2.0], np.float32) * len(self.calls)))
        out['linear'] = _Dev(lin_specs.reshape(B, S * self.hparams.reduction, -1)) if want_linear else None
        return out


def _write_dataset(root, rows, r, n_mels, F):
    os.makedirs(os.path.join(root, 'wavs'), exist_ok=True)
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for file_id, text in rows:
            f.write('{}|{}|{}\n'.format(file_id, text.upper(), text))
    rng = np.random.default_rng(0)
    feats = {}
    for i, (file_id, _) in enumerate(rows):
        t_red = 2 + i % 4
        mel = rng.random((t_red, n_mels * r)).astype(np.float32)
        lin = rng.random((t_red, F * r)).astype(np.float32)
        feats[file_id] = (mel, lin)
        np.savez(os.path.join(root, 'wavs', file_id + '.npz'), mel_mag_db=mel, linear_mag_db=lin)
    return feats


@pytest.mark.parametrize('linear', [False, True])
def test_gta_files_crop_name_and_pair_with_their_recordings(tmp_path, monkeypatch, hparams, linear):
    G = pkg('tacotron.gta')
    P = pkg('tacotron.params')
    monkeypatch.setattr(P.evaluation_params, 'n_buckets', 2)
    hp = copy.deepcopy(hparams)
    hp.reduction, hp.n_mels = 2, 4
    F = 3
    rows = [('LJ00{}'.format(i), text) for i, text in
            enumerate(['a cat', 'hi there', 'a longer sentence', 'dogs', 'mr. smith', 'ok', 'the end'])]
    feats = _write_dataset(str(tmp_path / 'data'), rows, hp.reduction, hp.n_mels, F)
    dataset = pkg('datasets.lj_speech').LJSpeechDatasetHelper(str(tmp_path / 'data'), P.dataset_params.vocabulary_dict,
                                                               False)
    model = _StubModel(hp)
    out_dir = str(tmp_path / 'gta')
    res = G.write_gta(model, G.batches_with_paths(dataset, None, 3, verbose=False), out_dir, with_linear=linear,
                      verbose=False)
    n_batches = len(model.calls)
    assert res['n_files'] == len(rows) and res['n_batches'] == n_batches >= 3
    # losses: unweighted mean over the batches
    assert res['loss_decoder'] == pytest.approx(np.mean(np.arange(1, n_batches + 1)))
    assert sorted(os.listdir(out_dir)) == sorted(fid + '.gta.npz' for fid, _ in rows)
    _, lengths, paths = dataset.load()
    for (fid, _), n_sent in zip(rows, lengths):
        with np.load(os.path.join(out_dir, fid + '.gta.npz')) as z:
            mel, lin = feats[fid]
            assert set(z.files) == {'mel_mag_db', 'alignments', 'durations'} | ({'linear_mag_db'} if linear else set())
            assert np.array_equal(z['mel_mag_db'], mel)   # its own recording, cropped to its own frames
            if linear:
                assert np.array_equal(z['linear_mag_db'], lin)
            assert z['alignments'].shape == (mel.shape[0], n_sent)
            d = z['durations']
            assert d.dtype == np.int32 and d.shape == (n_sent,) and d.sum() == mel.shape[0] * hp.reduction
            assert np.array_equal(d, G.durations(z['alignments'], hp.reduction))
