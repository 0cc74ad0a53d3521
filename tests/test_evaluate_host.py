"""CPU: the host side of Mode.EVAL -- bucketing and padding of tacotron/evaluate.py, the checkpoint listing, the LJ-Speech
listing reader and the pre-computed feature loader (reference tacotron/evaluate.py:18-151,284-326,
datasets/lj_speech.py:62-103, datasets/dataset_helper.py:285-305)."""
import os

import numpy as np
import pytest

from conftest import pkg


def _ev():
    return pkg('tacotron.evaluate')


def _reference_boundaries(lengths, n_buckets):
    # restatement of reference tacotron/evaluate.py:86-99
    s = np.sort(lengths)
    step = len(lengths) // n_buckets
    return sorted(list(set(s[::step][1:-1].tolist())))


@pytest.mark.parametrize('seed,n,n_buckets', [(0, 40, 20), (1, 1024, 20), (2, 57, 7), (3, 20, 20)])
def test_bucket_boundaries_match_the_reference_formula(seed, n, n_buckets):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(5, 30, n).tolist()     # few distinct values: duplicates are certain
    got = _ev().bucket_boundaries(lengths, n_buckets)
    assert got == _reference_boundaries(lengths, n_buckets)
    assert got == sorted(set(got))


def test_bucket_boundaries_duplicates_and_too_few_entries():
    ev = _ev()
    assert ev.bucket_boundaries([7] * 30, 10) == [7]
    assert ev.bucket_boundaries(list(range(10)), 5) == [2, 4, 6]   # sorted[::2] = 0 2 4 6 8 -> [1:-1]
    with pytest.raises(AssertionError):
        ev.bucket_boundaries([3, 4, 5], 4)


def test_bucket_batches_order_and_smaller_batches():
    ev = _ev()
    lengths = [10, 3, 12, 4, 11, 3, 20, 13, 5, 21]
    boundaries = [5, 12]          # buckets: < 5 | [5, 12) | >= 12
    got = ev.bucket_batches(lengths, boundaries, 2, allow_smaller_batches=True)
    # bucket 0: 1, 3, 5 -> [1, 3] + leftover [5]; bucket 1: 0, 4, 8 -> [0, 4] + [8]; bucket 2: 2, 6, 7, 9 -> [2, 6], [7, 9]
    assert got == [[1, 3], [0, 4], [2, 6], [7, 9], [5], [8]]
    assert ev.bucket_batches(lengths, boundaries, 2, allow_smaller_batches=False) == [[1, 3], [0, 4], [2, 6], [7, 9]]
    # a length equal to a boundary belongs to the bucket above it (TF: buckets_min <= L < buckets_max)
    assert ev.bucket_batches([5, 4], [5], 1) == [[1], [0]]


def test_pad_batch_pads_ids_with_zero_and_spectrograms_with_zero_frames():
    ev = _ev()
    s = [np.array([3, 4, 1], np.int32), np.array([5, 6, 7, 8, 1], np.int32)]
    f = [(np.full((2, 6), 0.5, np.float32), np.full((2, 9), 0.25, np.float32)),
         (np.full((4, 6), 0.75, np.float32), np.full((4, 9), 0.125, np.float32))]
    feed = ev.pad_batch(s, [3, 5], f)
    assert feed['ph_sentences'].dtype == np.int32
    assert feed['ph_sentences'].tolist() == [[3, 4, 1, 0, 0], [5, 6, 7, 8, 1]]
    assert feed['ph_sentence_length'].tolist() == [3, 5]
    assert feed['ph_time_frames'].tolist() == [2, 4]
    assert feed['ph_mel_specs'].shape == (2, 4, 6) and feed['ph_lin_specs'].shape == (2, 4, 9)
    assert np.all(feed['ph_mel_specs'][0, :2] == 0.5) and np.all(feed['ph_mel_specs'][0, 2:] == 0)
    assert np.all(feed['ph_lin_specs'][0, 2:] == 0) and np.all(feed['ph_lin_specs'][1] == 0.125)


def _write_dataset(root, rows, r=5, n_mels=4, F=3, skip_npz=()):
    """metadata.csv + wavs/<id>.npz with mel (T_red, n_mels*r) / linear (T_red, F*r); no .wav is needed."""
    os.makedirs(os.path.join(root, 'wavs'), exist_ok=True)
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for file_id, text in rows:
            f.write('{}|{}|{}\n'.format(file_id, text.upper(), text))
    rng = np.random.default_rng(0)
    feats = {}
    for i, (file_id, _) in enumerate(rows):
        t_red = 1 + i % 3
        mel = rng.random((t_red, n_mels * r)).astype(np.float32)
        lin = rng.random((t_red, F * r)).astype(np.float32)
        feats[file_id] = (mel, lin)
        if file_id not in skip_npz:
            np.savez(os.path.join(root, 'wavs', file_id + '.npz'), mel_mag_db=mel, linear_mag_db=lin)
    return feats


def _helper(root):
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper(str(root), P.dataset_params.vocabulary_dict, False)


def test_ljspeech_load_min_max_len_and_max_samples(tmp_path):
    rows = [('LJ001', 'a cat'), ('LJ002', 'hi'), ('LJ003', 'a longer sentence here'), ('LJ004', 'mr. smith'),
            ('LJ005', 'dogs')]
    _write_dataset(str(tmp_path), rows)
    ids, lengths, paths = _helper(tmp_path).load()
    assert len(ids) == 5 and paths[0] == os.path.join(str(tmp_path), 'wavs', 'LJ001.wav')
    assert np.frombuffer(ids[0], np.int32).tolist()[-1] == 1          # EOS appended
    assert lengths[0] == len('a cat') + 1
    assert lengths[3] == len('mister smith') + 1                      # abbreviations expanded after the length filter
    _, lengths, paths = _helper(tmp_path).load(min_len=4, max_len=10)
    assert [os.path.basename(p) for p in paths] == ['LJ001.wav', 'LJ004.wav', 'LJ005.wav']
    _, _, paths = _helper(tmp_path).load(max_samples=2, min_len=3)
    assert [os.path.basename(p) for p in paths] == ['LJ001.wav', 'LJ003.wav']
    _, _, paths = _helper(tmp_path).load(listing_file_name='metadata.csv', max_samples=1)
    assert len(paths) == 1


def test_npz_features_and_missing_npz_error(tmp_path):
    rows = [('LJ001', 'a cat'), ('LJ002', 'hi there'), ('LJ003', 'dogs')]
    feats = _write_dataset(str(tmp_path), rows, skip_npz=('LJ003',))
    h = _helper(tmp_path)
    _, _, paths = h.load()
    mel, lin = h.load_audio(paths[1])
    assert mel.dtype == np.float32 and np.array_equal(mel, feats['LJ002'][0]) and np.array_equal(lin, feats['LJ002'][1])
    mel, _ = h.load_audio(paths[0].encode())                          # the reference passes bytes through tf.py_func
    assert np.array_equal(mel, feats['LJ001'][0])
    cache = h.cache_precalculated_features(paths[:2])
    assert np.array_equal(cache[os.path.splitext(paths[0])[0]]['linear_mag_db'], feats['LJ001'][1])
    with pytest.raises(FileNotFoundError, match='LJ003.npz'):
        h.load_audio(paths[2])


def test_batched_placeholders_end_to_end_on_host(tmp_path):
    rows = [('LJ{:03d}'.format(i), 'word ' * (1 + i % 4)) for i in range(10)]
    feats = _write_dataset(str(tmp_path), rows)
    ev = _ev()
    batches = list(ev.batched_placeholders(_helper(tmp_path), None, 3, n_buckets=5, verbose=False))
    assert sum(b['ph_sentences'].shape[0] for b in batches) == 10
    seen = []
    for b in batches:
        B = b['ph_sentences'].shape[0]
        assert 1 <= B <= 3
        assert b['ph_mel_specs'].shape == (B, int(b['ph_time_frames'].max()), 20)
        for k in range(B):
            L = int(b['ph_sentence_length'][k])
            assert np.all(b['ph_sentences'][k, L:] == 0) and b['ph_sentences'][k, L - 1] == 1
            t = int(b['ph_time_frames'][k])
            assert np.all(b['ph_lin_specs'][k, t:] == 0)
            seen.append(b['ph_mel_specs'][k, :t].tobytes())
    assert sorted(seen) == sorted(v[0].tobytes() for v in feats.values())
    with pytest.raises(AssertionError):
        list(ev.batched_placeholders(_helper(tmp_path), None, 3, n_buckets=11, verbose=False))


def test_collect_checkpoint_paths_and_global_step(tmp_path):
    ev = _ev()
    (tmp_path / 'checkpoint').write_text('model_checkpoint_path: "model.ckpt-30"\n'
                                         'all_model_checkpoint_paths: "model.ckpt-10"\n'
                                         'all_model_checkpoint_paths: "model.ckpt-20"\n'
                                         'all_model_checkpoint_paths: "model.ckpt-30"\n')
    paths = ev.collect_checkpoint_paths(str(tmp_path))
    assert paths == [os.path.join(str(tmp_path), 'model.ckpt-{}'.format(s)) for s in (10, 20, 30)]
    assert [ev.global_step_of(p) for p in paths] == [10, 20, 30]
    assert ev.global_step_of('/some/dir-with-dash/model.ckpt-510000') == 510000


def test_evaluation_params_defaults_and_train_mode_still_refused():
    P = pkg('tacotron.params')
    e = P.evaluation_params
    assert (e.batch_size, e.max_samples, e.n_buckets, e.shuffle_samples, e.allow_smaller_batches) == (32, 1024, 20, False, True)
    assert (e.checkpoint_load_run, e.checkpoint_save_run, e.evaluate_all_checkpoints) == ('train', 'evaluate', False)
    M = pkg('tacotron.model')
    with pytest.raises(NotImplementedError):
        M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.TRAIN)


def test_evaluate_symbol_is_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'sstts_hip.h')) as f:
        assert 'int tts_evaluate(' in f.read()
    assert 'tts_evaluate' in pkg().exported_symbols()
