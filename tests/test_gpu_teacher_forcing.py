"""GPU: teacher forcing -- tts_decoder_forward_teacher / tts_teacher_forced (reference tacotron/helpers.py:208-405,
TacotronTrainingHelper) in both decoder forms (launch per layer, decoder.hip; the weight-stationary kernel's teacher variant,
decoder_ws.hip, with 16 and 32 utterances per cluster) against the float64 restatement of tests/teacher_oracle.py, against
the free-running decoder fed its own output, bit for bit across forms, batches and calls, and the losses of the call's own
outputs."""
import copy

import numpy as np
import pytest

from conftest import pkg, rel_l2
from parity import BTC, assert_alignment_rows, assert_mel_parity, assert_parity
import teacher_oracle as TO

pytestmark = pytest.mark.gpu

# (persistent_decoder, rows per cluster): what tts_teacher_kernel_choice reports for the form
FORMS = {'launch-per-layer': ((0, 0), 0), 'weight-stationary-16': ((1, 16), 2), 'weight-stationary-32': ((1, 32), 2)}


def _form(eng, name):
    (pd, rows), _ = FORMS[name]
    eng.set_option('persistent_decoder', pd)
    eng.set_option('debug_hooks', 1)
    eng.set_option('pd_rows', rows)


def _config(hparams, weights, name):
    hp = copy.deepcopy(hparams)
    w = weights
    if name == 'cudnn':
        hp.force_cudnn = True
    elif name == 'monotonic':
        hp.attention.mechanism = 'LocalLuongAttention'
        hp.attention.luong_local_window_D = 4
    elif name == 'predictive':
        hp.attention.mechanism = 'LocalLuongAttention'
        hp.attention.luong_local_mode = 'predictive'
        hp.attention.luong_local_window_D = 5
        hp.attention.luong_force_gaussian = False
    elif name == 'no_post':
        hp.apply_post_processing = False
    if name != 'global':
        w = pkg('tacotron.weights').synthetic_weights(11 if name == 'predictive' else 3, hp)
    return hp, w


def _engine(hp, w):
    eng = pkg().Engine(hp)
    eng.load_weights(w)
    return eng


def _w64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def _memory(B, Ts, seed, scale=0.5):
    return (np.random.default_rng(seed).standard_normal((B, Ts, 256)) * scale).astype(np.float32)


def _target(hp, B, S, seed):
    """normalised-dB-like mel targets (B, S, r*n_mels) in [0, 1)"""
    return np.random.default_rng(seed).random((B, S, hp.reduction * hp.n_mels)).astype(np.float32)


def _ids(B, Ts, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, Ts), np.int32)
    for b in range(B):
        L = int(rng.integers(max(2, Ts // 2), Ts + 1))
        ids[b, :L - 1] = rng.integers(2, 39, L - 1)
        ids[b, L - 1] = 1
    return ids


@pytest.mark.parametrize('config', ['global', 'cudnn', 'monotonic', 'predictive'])
@pytest.mark.parametrize('form', list(FORMS))
def test_teacher_decoder_vs_oracle(hparams, weights, config, form):
    """Both decoder forms, both GRU formulations, global / monotonic / predictive attention against the float64 restatement;
    batch sizes that fill no cluster."""
    hp, w = _config(hparams, weights, config)
    eng = _engine(hp, w)
    try:
        _form(eng, form)
        B, Ts, S = 5, 41, 9
        assert eng.teacher_kernel_choice(B, Ts) == FORMS[form][1]
        memory = _memory(B, Ts, 1)
        target = _target(hp, B, S, 2)
        ref_mel, ref_al = TO.decoder_teacher(memory.astype(np.float64), target.astype(np.float64), _w64(w), hp)
        mel, al = eng.decoder_forward_teacher(memory, target)
        label = 'teacher {} {}'.format(config, form)
        assert_mel_parity(mel.to_host(), ref_mel, 1e-3, label)
        assert_alignment_rows(al.to_host(), ref_al, 1e-4, label)
    finally:
        eng.close()


@pytest.mark.parametrize('config', ['global', 'no_post'])
@pytest.mark.parametrize('form', ['launch-per-layer', 'weight-stationary-16'])
def test_teacher_forced_network_vs_oracle(hparams, weights, config, form):
    """The whole network (encoder, teacher-forced decoder, post-net or -- apply_post_processing 0 -- the final Dense alone)
    against the restatement; the losses are the float64 L1 of the call's own returned outputs."""
    hp, w = _config(hparams, weights, config)
    eng = _engine(hp, w)
    try:
        _form(eng, form)
        B, Ts, S = 3, 17, 6
        ids = _ids(B, Ts, 4)
        target = _target(hp, B, S, 5)
        F = 1 + hp.n_fft // 2
        lin_t = np.random.default_rng(6).random((B, S, hp.reduction * F)).astype(np.float32)
        out = eng.teacher_forced(ids, target, lin_t, want_sums=True)
        ref_mel, ref_al, ref_lin = TO.teacher_forced(ids, target.astype(np.float64), _w64(w), hp)
        mel, al, lin = out['mel'].to_host(), out['alignments'].to_host(), out['linear'].to_host()
        label = 'teacher network {} {}'.format(config, form)
        assert_parity(mel, ref_mel, BTC, 1e-3, label + ' mel')
        assert_alignment_rows(al, ref_al, 1e-4, label)
        assert_parity(lin, ref_lin, BTC, 1e-3, label + ' linear')
        # per-utterance sums: float32 differences summed in float64 (eval_loss.hip), then the float64 L1 of the outputs
        sums = out['l1_sums'].to_host()
        d_mel, d_lin = np.abs(target.reshape(mel.shape) - mel), np.abs(lin_t.reshape(lin.shape) - lin)
        own32 = np.stack([d_mel.astype(np.float64).sum(axis=(1, 2)), d_lin.astype(np.float64).sum(axis=(1, 2))], -1)
        np.testing.assert_allclose(sums, own32, rtol=1e-11)
        own = np.stack([np.abs(target.reshape(mel.shape).astype(np.float64) - mel).sum(axis=(1, 2)),
                        np.abs(lin_t.reshape(lin.shape).astype(np.float64) - lin).sum(axis=(1, 2))], -1)
        np.testing.assert_allclose(sums, own, rtol=1e-7)
        dec, post = own[:, 0].sum() / mel.size, own[:, 1].sum() / lin.size
        losses = out['losses'].to_host()
        assert abs(losses[1] - dec) <= 1e-6 * dec and abs(losses[2] - post) <= 1e-6 * post
        assert losses[0] == np.float32(losses[1]) + np.float32(losses[2])
        # no linear target: no losses, the same spectrograms
        bare = eng.teacher_forced(ids, target)
        assert bare['losses'] is None and bare['l1_sums'] is None
        assert np.array_equal(bare['mel'].to_host(), mel) and np.array_equal(bare['linear'].to_host(), lin)
    finally:
        eng.close()


def test_teacher_full_size_b64(engine, hparams, weights64):
    """B = 64, T_s = 150, S = 200 through the default form (weight-stationary, 16 rows) against the restatement."""
    _form(engine, 'weight-stationary-16')
    try:
        B, Ts, S = 64, 150, 200
        memory = _memory(B, Ts, 7)
        target = _target(hparams, B, S, 8)
        ref_mel, ref_al = TO.decoder_teacher(memory.astype(np.float64), target.astype(np.float64), weights64, hparams)
        mel, al = engine.decoder_forward_teacher(engine.to_device(memory), engine.to_device(target))
        assert_mel_parity(mel.to_host(), ref_mel, 1e-3, 'teacher B=64 S=200')
        assert_alignment_rows(al.to_host(), ref_al, 1e-4, 'teacher B=64 S=200')
    finally:
        engine.set_option('persistent_decoder', 1)
        engine.set_option('pd_rows', 0)
        engine.set_option('debug_hooks', 0)


@pytest.mark.parametrize('form', list(FORMS))
def test_fed_its_own_output_it_reproduces_the_free_run(engine, form):
    """Fed the free-running call's own mel, the teacher-forced call reproduces it within float rounding (the free path folds
    the output projection into the pre-net matrix: not the same bits)."""
    _form(engine, form)
    try:
        B, Ts, S = 4, 30, 12
        memory = engine.to_device(_memory(B, Ts, 9))
        free_mel, free_al = engine.decoder_forward(memory, S)
        free_mel, free_al = free_mel.to_host(), free_al.to_host()
        mel, al = engine.decoder_forward_teacher(memory, free_mel)
        assert_mel_parity(mel.to_host(), free_mel, 1e-4, 'teacher vs free ' + form)
        assert_alignment_rows(al.to_host(), free_al, 1e-4, 'teacher vs free ' + form)
    finally:
        engine.set_option('persistent_decoder', 1)
        engine.set_option('pd_rows', 0)
        engine.set_option('debug_hooks', 0)


@pytest.mark.parametrize('form', list(FORMS))
def test_bits_do_not_depend_on_batch_position_rows_or_history(engine, hparams, form):
    """Given the padded shape, an utterance's bits do not depend on the batch size, its position, the rows per cluster
    (16 / 32: the same bits) or the calls the handle ran before; a free-running call's bits do not change after a
    teacher-forced call."""
    B, Ts, S = 37, 26, 7
    memory = _memory(B, Ts, 10)
    target = _target(hparams, B, S, 11)
    try:
        _form(engine, form)
        free0 = engine.decoder_forward(memory, S)[0].to_host()
        mel0, al0 = [a.to_host() for a in engine.decoder_forward_teacher(memory, target)]
        if form != 'launch-per-layer':   # the other row count of the weight-stationary kernel: the same bits
            other = 'weight-stationary-32' if form == 'weight-stationary-16' else 'weight-stationary-16'
            _form(engine, other)
            mel1, al1 = [a.to_host() for a in engine.decoder_forward_teacher(memory, target)]
            assert np.array_equal(mel1, mel0) and np.array_equal(al1, al0)
            _form(engine, form)
        # a sub-batch, reversed: other positions, another batch size (one cluster instead of several)
        idx = np.array([36, 20, 5, 0])
        mel2, al2 = [a.to_host() for a in engine.decoder_forward_teacher(memory[idx], target[idx])]
        assert np.array_equal(mel2, mel0[idx]) and np.array_equal(al2, al0[:, idx])
        # a single utterance after a full synthesis-sized free call
        engine.decoder_forward(_memory(64, 60, 12), 20)
        mel3, al3 = [a.to_host() for a in engine.decoder_forward_teacher(memory[17:18], target[17:18])]
        assert np.array_equal(mel3, mel0[17:18]) and np.array_equal(al3, al0[:, 17:18])
        # the free-running call is unchanged by the teacher-forced calls
        assert np.array_equal(engine.decoder_forward(memory, S)[0].to_host(), free0)
        assert np.array_equal(engine.decoder_forward_teacher(memory, target)[0].to_host(), mel0)
    finally:
        engine.set_option('persistent_decoder', 1)
        engine.set_option('pd_rows', 0)
        engine.set_option('debug_hooks', 0)


def test_the_last_group_is_never_fed(engine, hparams):
    """Changing the last r target frames changes nothing; changing frame t*r - 1 leaves the steps before t unchanged."""
    B, Ts, S, r = 3, 20, 6, hparams.reduction
    memory = engine.to_device(_memory(B, Ts, 13))
    target = _target(hparams, B, S, 14)
    mel0 = engine.decoder_forward_teacher(memory, target)[0].to_host()
    t2 = target.copy()
    t2[:, -1, :] += 1.0
    assert np.array_equal(engine.decoder_forward_teacher(memory, t2)[0].to_host(), mel0)
    t3 = target.reshape(B, S * r, -1).copy()
    t3[:, 3 * r - 1] += 1.0
    mel3 = engine.decoder_forward_teacher(memory, t3)[0].to_host()
    assert np.array_equal(mel3[:, :3], mel0[:, :3]) and not np.array_equal(mel3[:, 3], mel0[:, 3])


def test_edge_cases_and_refusals(engine, hparams, weights):
    """S = 1 and B = 1; bad arguments are refused; LocalLuongAttention keeps its refusals (memory shorter than 2D+1, a
    predicted window that leaves the memory)."""
    H = pkg('_hip')
    memory = _memory(1, 9, 15)
    target = _target(hparams, 1, 1, 16)
    mel, al = engine.decoder_forward_teacher(memory, target)
    free_mel, free_al = engine.decoder_forward(memory, 1)
    # one step reads only the GO frame: the free run's first step (within rounding: the folded projection is not used)
    assert rel_l2(mel.to_host(), free_mel.to_host()) < 1e-5 and rel_l2(al.to_host(), free_al.to_host()) < 1e-5
    with pytest.raises(ValueError):
        engine.decoder_forward_teacher(memory, target[:, :, :7])
    dmem = engine.to_device(memory)
    dtgt = engine.to_device(_target(hparams, 1, 3, 17))
    dmel = engine.empty((1, 3, hparams.reduction * hparams.n_mels))
    lib, h = engine.lib, engine.handle
    assert lib.tts_decoder_forward_teacher(h, dmem.ptr, 1, 9, 3, None, dmel.ptr, None) == H.TTS_ERR_INVALID
    assert lib.tts_decoder_forward_teacher(h, dmem.ptr, 1, 9, 0, dtgt.ptr, dmel.ptr, None) == H.TTS_ERR_INVALID
    assert lib.tts_decoder_forward_teacher(h, dmem.ptr, 1, 9, 2, dtgt.ptr + 4, dmel.ptr, None) == H.TTS_ERR_INVALID
    ids = engine.to_device(np.ones((1, 9), np.int32))
    assert lib.tts_teacher_forced(h, ids.ptr, 1, 9, 3, None, None, None, None, None, None, None) == H.TTS_ERR_INVALID
    assert lib.tts_teacher_forced(h, ids.ptr, 1, 9, 3, dtgt.ptr, dtgt.ptr, None, None, None, None, None) == H.TTS_ERR_INVALID
    assert lib.tts_teacher_kernel_choice(h, 0, 9) == H.TTS_ERR_INVALID
    # LocalLuongAttention: memory shorter than 2D+1
    hp, w = _config(hparams, weights, 'monotonic')
    eng = _engine(hp, w)
    try:
        with pytest.raises(H.TtsError) as ei:
            eng.decoder_forward_teacher(_memory(2, 8, 18), _target(hp, 2, 3, 19))
        assert ei.value.code == H.TTS_ERR_UNSUPPORTED
    finally:
        eng.close()
    # predictive: T_s = 2D+1 and a large v_p spread the predicted centres beyond the memory
    hp, w = _config(hparams, weights, 'predictive')
    hp.attention.luong_local_window_D = 10
    vp = 'decoder2/decoder/output_projection_wrapper/multi_rnn_cell/cell_0/attention_wrapper/local_luong_attention/local_v_p'
    w = dict(w)
    w[vp] = (w[vp] * 8.0).astype(np.float32)
    eng = _engine(hp, w)
    try:
        for form in ('launch-per-layer', 'weight-stationary-16'):
            _form(eng, form)
            with pytest.raises(H.TtsError) as ei:
                eng.decoder_forward_teacher(np.random.default_rng(1).standard_normal((2, 21, 256)).astype(np.float32),
                                            _target(hp, 2, 3, 20))
            assert ei.value.code == H.TTS_ERR_UNSUPPORTED
    finally:
        eng.close()
