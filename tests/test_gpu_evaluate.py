"""GPU: Mode.EVAL -- tts_evaluate (encoder, free-running decoder, post-net, L1 losses of csrc/eval_loss.hip) against the
float64 oracle composed from oracle.tacotron_oracle, against the stand-alone stages, bit for bit across calls, and the
Python layers above it (reference tacotron/model.py:299-306,432-442, tacotron/evaluate.py:153-257)."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import pkg
from tf_bundle_writer import write_tensor_bundle

pytestmark = pytest.mark.gpu


def _ids(B, Ts, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, Ts), np.int32)
    for b in range(B):
        L = int(rng.integers(max(2, Ts // 2), Ts))
        ids[b, :L - 1] = rng.integers(2, 39, L - 1)
        ids[b, L - 1] = 1
    return ids


def _targets(hp, B, S, seed, tail=True):
    """normalised-dB-like targets (B, S, r*n_mels) / (B, S, r*F) whose last frames are zero padding"""
    rng = np.random.default_rng(seed)
    r, F = hp.reduction, 1 + hp.n_fft // 2
    mel = rng.random((B, S * r, hp.n_mels)).astype(np.float32)
    lin = rng.random((B, S * r, F)).astype(np.float32)
    if tail:
        for b in range(B):
            keep = max(1, S * r - 3 * (b + 1))
            mel[b, keep:] = 0
            lin[b, keep:] = 0
    return mel.reshape(B, S, r * hp.n_mels), lin.reshape(B, S, r * F)


def _oracle_losses(ids, mel_t, lin_t, w64, hp):
    O = pytest.importorskip('oracle.tacotron_oracle')
    B = ids.shape[0]
    S = mel_t.shape[1]
    memory = O.encoder(ids, w64, hp)
    red, _ = O.decoder(memory, w64, hp, n_steps=S)
    mel = red.reshape(B, -1, hp.n_mels)
    lin = O.post_process(mel, w64, hp) if hp.apply_post_processing else O.dense(mel, w64, 'dense')
    dec = np.mean(np.abs(mel_t.reshape(mel.shape).astype(np.float64) - mel))
    post = np.mean(np.abs(lin_t.reshape(lin.shape).astype(np.float64) - lin))
    return np.array([dec + post, dec, post])


def _config(hparams, weights, name):
    hp = copy.deepcopy(hparams)
    w = weights
    if name == 'cudnn':
        hp.force_cudnn = True
    elif name == 'local':
        hp.attention.mechanism = 'LocalLuongAttention'
        hp.attention.luong_local_window_D = 4
    elif name == 'no_post':
        hp.apply_post_processing = False
    elif name == 'n_fft_512':
        hp.n_fft = 512
    if name != 'default':
        w = pkg('tacotron.weights').synthetic_weights(3, hp)
    return hp, w


@pytest.mark.parametrize('name', ['default', 'cudnn', 'local', 'no_post', 'n_fft_512'])
def test_losses_match_the_float64_oracle(hparams, weights, name):
    hp, w = _config(hparams, weights, name)
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        B, Ts, S = 3, 17, 6
        ids = _ids(B, Ts, 1)
        mel_t, lin_t = _targets(hp, B, S, 2)
        got = eng.evaluate(ids, mel_t, lin_t)['losses'].to_host()
        ref = _oracle_losses(ids, mel_t, lin_t, {k: v.astype(np.float64) for k, v in w.items()}, hp)
        print('{}: losses {} oracle {}'.format(name, got, ref))
        assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref)), (got, ref)
        assert got[0] == np.float32(got[1]) + np.float32(got[2])
    finally:
        eng.close()


def _l1(a, b):
    return np.sum(np.abs(a.astype(np.float64) - b.astype(np.float64)))


def test_self_consistency_with_the_stand_alone_stages(engine, hparams):
    B, Ts, S = 4, 23, 7
    ids = _ids(B, Ts, 5)
    mel_t, lin_t = _targets(hparams, B, S, 6)
    memory = engine.encoder_forward(ids)
    mel_ref, _ = engine.decoder_forward(memory, S, want_alignments=False)
    mel_ref.shape = (B, S * hparams.reduction, hparams.n_mels)
    lin_ref = engine.postnet_forward(mel_ref).to_host()
    mel_ref = mel_ref.to_host()
    out = engine.evaluate(ids, mel_t, lin_t, want_sums=True, want_mel=True, want_linear=True, want_alignments=True)
    assert np.array_equal(out['mel'].to_host(), mel_ref)
    assert np.array_equal(out['linear'].to_host(), lin_ref)
    T = S * hparams.reduction
    m64 = mel_t.reshape(B, T, -1)
    l64 = lin_t.reshape(B, T, -1)
    sums = out['l1_sums'].to_host()
    for b in range(B):
        assert abs(sums[b, 0] - _l1(m64[b], mel_ref[b])) <= 1e-9 * sums[b, 0]
        assert abs(sums[b, 1] - _l1(l64[b], lin_ref[b])) <= 1e-9 * sums[b, 1]
    losses = out['losses'].to_host()
    dec = _l1(m64, mel_ref) / m64.size
    post = _l1(l64, lin_ref) / l64.size
    assert abs(losses[1] - dec) <= 1e-6 * dec and abs(losses[2] - post) <= 1e-6 * post
    # targets = the stand-alone outputs: everything is exactly zero
    z = engine.evaluate(ids, mel_ref.reshape(B, S, -1), lin_ref.reshape(B, S, -1), want_sums=True)
    assert np.all(z['losses'].to_host() == 0.0)
    assert np.all(z['l1_sums'].to_host() == 0.0)


def test_misaligned_target_buffers(engine, hparams):
    """targets that start 4 bytes past a 16-byte boundary (the element-wise path for the output slabs)"""
    B, Ts, S = 2, 15, 5
    ids = _ids(B, Ts, 8)
    mel_t, lin_t = _targets(hparams, B, S, 9)
    out = engine.evaluate(ids, mel_t, lin_t, want_sums=True, want_mel=True, want_linear=True)
    mel_o, lin_o = out['mel'].to_host(), out['linear'].to_host()
    dm = engine.to_device(np.concatenate([[0.0], mel_t.reshape(-1)]).astype(np.float32))
    dl = engine.to_device(np.concatenate([[0.0], lin_t.reshape(-1)]).astype(np.float32))
    loss = engine.empty((3,))
    sums = engine.empty((B, 2), np.float64)
    p_ids = engine.to_device(ids)
    engine._check(engine.lib.tts_evaluate(engine.handle, p_ids.ptr, B, Ts, S, dm.ptr + 4, dl.ptr + 4, loss.ptr, sums.ptr,
                                          None, None, None))
    s = sums.to_host()
    T = S * hparams.reduction
    for b in range(B):
        assert abs(s[b, 0] - _l1(mel_t.reshape(B, T, -1)[b], mel_o[b])) <= 1e-9 * s[b, 0]
        assert abs(s[b, 1] - _l1(lin_t.reshape(B, T, -1)[b], lin_o[b])) <= 1e-9 * s[b, 1]
    assert np.allclose(loss.to_host(), out['losses'].to_host(), rtol=1e-6, atol=0)


def test_determinism_across_calls_and_shapes(engine, hparams):
    B, Ts, S = 5, 19, 6
    ids = _ids(B, Ts, 10)
    mel_t, lin_t = _targets(hparams, B, S, 11)
    dm, dl = engine.to_device(mel_t), engine.to_device(lin_t)
    first = engine.evaluate(ids, dm, dl, want_sums=True)
    l0, s0 = first['losses'].to_host(), first['l1_sums'].to_host()
    for _ in range(3):
        again = engine.evaluate(ids, dm, dl, want_sums=True)
        assert np.array_equal(again['losses'].to_host(), l0) and np.array_equal(again['l1_sums'].to_host(), s0)
    # differently shaped calls in between (bigger workspaces, other grids)
    ids2 = _ids(9, 31, 12)
    m2, l2 = _targets(hparams, 9, 11, 13)
    engine.evaluate(ids2, m2, l2)
    engine.evaluate(ids[:1], mel_t[:1, :2], lin_t[:1, :2])
    after = engine.evaluate(ids, dm, dl, want_sums=True)
    assert np.array_equal(after['losses'].to_host(), l0) and np.array_equal(after['l1_sums'].to_host(), s0)


def test_beside_gemm_launches_of_another_handle(engine, hparams, weights):
    eng2 = pkg().Engine(hparams)
    try:
        eng2.load_weights(weights)
        rng = np.random.default_rng(7)
        x = eng2.to_device(rng.standard_normal((9600, 256)).astype(np.float32))
        w = eng2.to_device(rng.standard_normal((256, 256)).astype(np.float32))
        c = eng2.empty((9600, 256))
        B, Ts, S = 8, 40, 8
        ids = _ids(B, Ts, 14)
        mel_t, lin_t = _targets(hparams, B, S, 15)
        dm, dl = engine.to_device(mel_t), engine.to_device(lin_t)
        quiet = engine.evaluate(ids, dm, dl, want_sums=True)
        lq, sq = quiet['losses'].to_host(), quiet['l1_sums'].to_host()
        for _ in range(30):
            eng2._check(eng2.lib.tts_debug_gemm(eng2.handle, x.data_ptr(), w.data_ptr(), c.data_ptr(), 9600, 256, 256, 1, 150, 0))
        busy = engine.evaluate(ids, dm, dl, want_sums=True)
        assert np.array_equal(busy['losses'].to_host(), lq) and np.array_equal(busy['l1_sums'].to_host(), sq)
        eng2.synchronize()
        for a in (x, w, c):
            a.free()
    finally:
        eng2.close()


def test_edge_cases(engine, hparams, weights64):
    # B = 1, n_steps = 1
    ids = _ids(1, 9, 16)
    mel_t, lin_t = _targets(hparams, 1, 1, 17, tail=False)
    got = engine.evaluate(ids, mel_t, lin_t)['losses'].to_host()
    ref = _oracle_losses(ids, mel_t, lin_t, weights64, hparams)
    assert np.all(np.abs(got - ref) <= 1e-5 * ref)
    # a NaN in a target gives a NaN loss
    ids = _ids(2, 11, 18)
    mel_t, lin_t = _targets(hparams, 2, 3, 19)
    bad = lin_t.copy()
    bad[1, 2, 7] = np.nan
    got = engine.evaluate(ids, mel_t, bad)['losses'].to_host()
    assert np.isnan(got[0]) and np.isnan(got[2]) and np.isfinite(got[1])
    bad = mel_t.copy()
    bad[0, 0, 0] = np.inf
    got = engine.evaluate(ids, bad, lin_t)['losses'].to_host()
    assert np.isinf(got[1]) and np.isinf(got[0])
    # NULL pointers and bad sizes
    TE = pkg().TtsError
    dm, dl, di = engine.to_device(mel_t), engine.to_device(lin_t), engine.to_device(ids)
    loss = engine.empty((3,))
    lib, h = engine.lib, engine.handle
    for args in [(None, 2, 11, 3, dm.ptr, dl.ptr, loss.ptr), (di.ptr, 2, 11, 3, None, dl.ptr, loss.ptr),
                 (di.ptr, 2, 11, 3, dm.ptr, None, loss.ptr), (di.ptr, 2, 11, 3, dm.ptr, dl.ptr, None),
                 (di.ptr, 0, 11, 3, dm.ptr, dl.ptr, loss.ptr), (di.ptr, 2, 0, 3, dm.ptr, dl.ptr, loss.ptr),
                 (di.ptr, 2, 11, 0, dm.ptr, dl.ptr, loss.ptr), (di.ptr, 2, 11, -1, dm.ptr, dl.ptr, loss.ptr),
                 (di.ptr, 2, 11, 3, dm.ptr + 2, dl.ptr, loss.ptr)]:
        rc = lib.tts_evaluate(h, *args, None, None, None, None)
        assert rc == pkg()._hip.TTS_ERR_INVALID, args
        assert lib.tts_last_error(h)
    with pytest.raises(ValueError):
        engine.evaluate(ids, mel_t[:, :, :7], lin_t)
    with pytest.raises(ValueError):
        engine.evaluate(ids, mel_t, lin_t[:, :2])
    # the handle still works after the refusals
    assert np.isfinite(engine.evaluate(ids, mel_t, lin_t)['losses'].to_host()).all()


def test_profile_stage(engine, hparams):
    ids = _ids(2, 11, 20)
    mel_t, lin_t = _targets(hparams, 2, 3, 21)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        engine.evaluate(ids, mel_t, lin_t)
        ms, n = engine.profile_get('eval_loss')
        assert n == 2 and ms > 0
    finally:
        engine.set_option('profile', 0)


def test_facade_mode_eval(hparams, weights):
    M = pkg('tacotron.model')
    ph = M.Tacotron.model_placeholders()
    model = M.Tacotron(ph, M.Mode.EVAL, weights=weights, hparams=hparams)
    try:
        B, Ts, S = 3, 14, 4
        ids = _ids(B, Ts, 22)
        mel_t, lin_t = _targets(hparams, B, S, 23)
        feed = {model.inp_sentences: ids, model.inp_mel_spec: mel_t, model.inp_linear_spec: lin_t,
                ph['ph_sentence_length']: np.array([5, 6, 7], np.int32), ph['ph_time_frames']: np.array([4, 3, 2], np.int32)}
        loss, dec, post = model.run([model.loss_op, model.loss_op_decoder, model.loss_op_post_processing], feed)
        eng = model.engine.evaluate(ids, mel_t, lin_t)['losses'].to_host()
        assert np.array_equal(np.array([loss, dec, post], np.float32), eng)
        assert np.float32(loss) == np.float32(dec) + np.float32(post)
        assert model.get_loss_op() is model.loss_op
        lin, red = model.run([model.output_linear_spec, model.reduced_output_mel_spec], feed)
        assert lin.shape == (B, S * hparams.reduction, 1 + hparams.n_fft // 2) and red.shape == mel_t.shape
    finally:
        model.engine.close()


def _dataset(root, hp, n=20):
    rng = np.random.default_rng(30)
    words = ['a', 'cat', 'sat', 'on', 'the', 'mat', 'dog', 'ran']
    os.makedirs(os.path.join(root, 'wavs'))
    F = 1 + hp.n_fft // 2
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for i in range(n):
            text = ' '.join(rng.choice(words, 1 + i % 4))
            fid = 'LJ{:03d}'.format(i)
            f.write('{}|{}|{}\n'.format(fid, text.upper(), text))
            t_red = 1 + int(rng.integers(0, 4))
            mel = rng.random((t_red, hp.n_mels * hp.reduction)).astype(np.float32)
            lin = rng.random((t_red, F * hp.reduction)).astype(np.float32)
            np.savez(os.path.join(root, 'wavs', fid + '.npz'), mel_mag_db=mel, linear_mag_db=lin)


def test_end_to_end_evaluate_and_cli(tmp_path, hparams, weights, weights64):
    C = pkg('tacotron.checkpoint')
    E = pkg('tacotron.evaluate')
    data = str(tmp_path / 'data')
    _dataset(data, hparams)
    run = tmp_path / 'ckpt' / 'train'
    run.mkdir(parents=True)
    ck = dict(weights)
    ck['global_step'] = np.array(1200, dtype=np.int64)
    write_tensor_bundle(str(run / 'model.ckpt-1200'), ck, block_entries=16, crc_fn=C.crc32c)
    (run / 'checkpoint').write_text('model_checkpoint_path: "model.ckpt-1200"\n'
                                    'all_model_checkpoint_paths: "model.ckpt-1200"\n')
    # numpy over the oracle, batch by batch
    P = pkg('tacotron.params')
    helper = pkg('datasets.lj_speech').LJSpeechDatasetHelper(data, P.dataset_params.vocabulary_dict, False)
    per_batch = [_oracle_losses(b['ph_sentences'], b['ph_mel_specs'], b['ph_lin_specs'], weights64, hparams)
                 for b in E.batched_placeholders(helper, 20, 4, verbose=False)]
    ref = np.mean(per_batch, axis=0)
    res = E.evaluate_checkpoint(str(run / 'model.ckpt-1200'), dataset_folder=data, max_samples=20, batch_size=4,
                                checkpoint_dir=str(tmp_path / 'ckpt'), hparams=hparams)
    assert res['global_step'] == 1200 and res['n_batches'] == len(per_batch)
    got = np.array([res['loss'], res['loss_decoder'], res['loss_post_processing']])
    print('evaluate: {} oracle {} over {} batches'.format(got, ref, len(per_batch)))
    assert np.all(np.abs(got - ref) <= 1e-5 * ref)
    with open(str(tmp_path / 'ckpt' / 'evaluate' / E.SUMMARY_FILE)) as f:
        line = json.loads(f.readline())
    assert line['global_step'] == 1200 and line['loss/loss'] == res['loss']
    # the CLI: latest checkpoint, and the sweep
    argv = ['--checkpoint-dir', str(tmp_path / 'ckpt'), '--dataset-folder', data, '--max-samples', '20', '--batch-size', '4']
    assert E.main(argv) == 0
    assert E.main(argv + ['--all']) == 0
    with open(str(tmp_path / 'ckpt' / 'evaluate' / E.SUMMARY_FILE)) as f:
        lines = [json.loads(l) for l in f]
    assert len(lines) == 3 and all(l['loss/loss'] == res['loss'] for l in lines)
