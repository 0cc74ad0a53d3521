"""GPU: the network at every architecture family tts_create accepts, against the float64 oracle.

The rest of the GPU suite runs the reference's architecture (plus other highway depths, force_cudnn, the attention mechanisms
and apply_post_processing).  tts_create takes far more -- n_mels, the embedding and pre-net widths, the bank and projection
filters, any number of conv banks, any reduction, any vocabulary, 1 to 4 decoder GRU layers -- and those fields reach index
arithmetic, tilings and kernel choices that the reference's numbers never exercise.  tests/arch_cases.py names a small table of
architectures, each there for particular branches (its docstring lists them); every one gets an engine of its own here and
is compared stage by stage, in every decoder form it admits, free-running and teacher-forced, and as a whole network, with the
bounds the suite already uses: stage intermediates 1e-4, memory / mel / linear 1e-3, every alignment row 1e-4, losses 1e-5.
tests/test_architectures_host.py shows on the CPU that float32 arithmetic keeps a fourfold margin to each of these bounds on
these inputs and that a wrong frame index or a dropped residual misses them a hundredfold.
"""
import numpy as np
import pytest

import arch_cases as C
from conftest import pkg, rel_l2
from parity import BTC, assert_alignment_rows, assert_mel_parity, assert_parity

pytestmark = pytest.mark.gpu

WIN, HOP = 1102, 275


@pytest.fixture(scope='module', params=list(C.ARCHS))
def net(request, hparams):
    """(name, hyper-parameters, engine) of one architecture; the engine lives for the architecture's tests."""
    name = request.param
    hp = C.configure(hparams, name)                       # copy.deepcopy(hparams) with the architecture's fields moved
    ref_hp, w, _ = C.arch(name)                           # synthetic_weights(seed_of(name), hp): shared with the references
    assert hp == ref_hp
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        yield name, hp, eng
    finally:
        eng.close()


def _set_form(eng, form):
    pd, pd_ws, rows = C.FORMS[form][0]
    eng.set_option('persistent_decoder', pd)
    eng.set_option('pd_ws', pd_ws)
    eng.set_option('debug_hooks', 1)
    eng.set_option('pd_rows', rows)


def _reset_form(eng):
    eng.set_option('pd_rows', 0)
    eng.set_option('debug_hooks', 0)
    eng.set_option('pd_ws', 1)
    eng.set_option('persistent_decoder', 1)


@pytest.mark.parametrize('B,Ts,unknown', [s + (False,) for s in C.ENC_SHAPES] + [C.ENC_SHAPES[1] + (True,)])
def test_encoder_stages(net, B, Ts, unknown):
    """Embedding gather, pre-net, bank (one launch per 16 banks), split-K or plain projection 1, projection 2 + residual, the
    CBHG tail (fused up to 128 input channels, else layer by layer) and the memory, at the architecture's own widths.
    ``unknown``: a device-resident id array with two ids outside the vocabulary, which read as zero embedding rows."""
    name, hp, eng = net
    enc = hp.encoder
    ids, ref, ref_mem = C.encoder_case(name, B, Ts, unknown)
    mem = eng.encoder_forward(eng.to_device(ids) if unknown else ids).to_host()
    P2, NBF, PF = enc.pre_net_layers[1][0], enc.n_banks * enc.n_filters, [p[0] for p in enc.projections]
    got = {
        'prenet': eng.debug_workspace('enc.pre2', (B, Ts, P2)),
        'bank': eng.debug_workspace('enc.bank', (B, Ts, NBF)),
        'proj1': eng.debug_workspace('enc.p1', (B, Ts, PF[0])),
        'proj2': eng.debug_workspace('enc.p2', (B, Ts, PF[1])),
        'highway': eng.debug_workspace('enc.hw0', (B, Ts, enc.n_highway_units)),
    }
    label = '{} encoder B={} Ts={}{}'.format(name, B, Ts, ' unknown ids' if unknown else '')
    for k, v in got.items():
        assert_parity(v, ref[k], BTC, C.STAGE_TOL, '{} {}'.format(label, k))
    assert_parity(mem, ref_mem, BTC, C.FINAL_TOL, label + ' memory')
    if P2 > 128:   # the fused tail does not cover this width: the option changes nothing, bit for bit
        eng.set_option('fused_tail', 0)
        try:
            assert np.array_equal(eng.encoder_forward(eng.to_device(ids) if unknown else ids).to_host(), mem)
        finally:
            eng.set_option('fused_tail', 1)


@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('B,T', C.POST_SHAPES)
def test_postnet_stages(net, B, T, fused):
    name, hp, eng = net
    post = hp.post
    mel, ref, ref_lin = C.postnet_case(name, B, T)

    def run(option):
        eng.set_option('fused_tail', option)
        try:
            lin = eng.postnet_forward(mel).to_host()
            return lin, {
                'bank': eng.debug_workspace('post.bank', (B, T, post.n_banks * post.n_filters)),
                'proj1': eng.debug_workspace('post.p1', (B, T, post.projections[0][0])),
                'highway': eng.debug_workspace('post.hw0', (B, T, post.n_highway_units)),
                'gru': eng.debug_workspace('post.gru', (B, T, 2 * post.n_gru_units)),
            }
        finally:
            eng.set_option('fused_tail', 1)

    lin, got = run(fused)
    label = '{} postnet fused={} B={} T={}'.format(name, fused, B, T)
    for k, v in got.items():
        assert_parity(v, ref[k], BTC, C.FINAL_TOL if k == 'gru' else C.STAGE_TOL, '{} {}'.format(label, k))
    assert_parity(lin, ref_lin, BTC, C.FINAL_TOL, label + ' linear')
    if hp.n_mels > 128 and not fused:   # cbhg_tail_supports says no (c_in > 128): both options are the layer-by-layer chain
        lin1, got1 = run(1)
        assert np.array_equal(lin1, lin)
        for k in got:
            assert np.array_equal(got1[k], got[k]), k


@pytest.mark.parametrize('form', list(C.FORMS))
@pytest.mark.parametrize('B,Ts,S', C.DEC_SHAPES)
def test_decoder_free_running(net, B, Ts, S, form):
    """Every decoder form the architecture admits -- and, where it is outside a persistent kernel, the launch-per-layer path
    taking over whatever the options ask for -- against the oracle; tts_decoder_kernel_choice says which kernel ran."""
    name, hp, eng = net
    memory, ref_mel, ref_al = C.decoder_case(name, B, Ts, S)
    _set_form(eng, form)
    try:
        choice = eng.decoder_kernel_choice(B, Ts, pipelined=False)
        print('{} decoder {} B={} Ts={} S={}: kernel choice {}'.format(name, form, B, Ts, S, choice))
        assert choice == C.expected_choice(hp, form)
        mel, al = eng.decoder_forward(memory, S)
        eng.synchronize()
        mel, al = mel.to_host(), al.to_host()
    finally:
        _reset_form(eng)
    label = '{} decoder {} (kernel {}) B={} Ts={} S={}'.format(name, form, choice, B, Ts, S)
    assert_mel_parity(mel, ref_mel, C.FINAL_TOL, label, n_mels=hp.n_mels)
    assert_alignment_rows(al, ref_al, C.ALIGN_TOL, label)
    assert np.allclose(al.sum(-1), 1.0, atol=1e-5)


@pytest.mark.parametrize('form', list(C.FORMS))
@pytest.mark.parametrize('B,Ts,S', C.DEC_SHAPES)
def test_decoder_teacher_forced(net, B, Ts, S, form):
    """tts_decoder_forward_teacher (frame t*r - 1 of the target at step t, row stride r * n_mels) against
    tests/teacher_oracle.py.  The streamed-weights kernel has no teacher form: under its options the call is the
    launch-per-layer one."""
    name, hp, eng = net
    memory, target, ref_mel, ref_al = C.teacher_case(name, B, Ts, S)
    _set_form(eng, form)
    try:
        choice = eng.teacher_kernel_choice(B, Ts)
        print('{} teacher decoder {} B={} Ts={} S={}: kernel choice {}'.format(name, form, B, Ts, S, choice))
        assert choice == C.expected_teacher_choice(hp, form)
        mel, al = eng.decoder_forward_teacher(memory, target)
        eng.synchronize()
        mel, al = mel.to_host(), al.to_host()
    finally:
        _reset_form(eng)
    label = '{} teacher decoder {} (kernel {}) B={} Ts={} S={}'.format(name, form, choice, B, Ts, S)
    assert_mel_parity(mel, ref_mel, C.FINAL_TOL, label, n_mels=hp.n_mels)
    assert_alignment_rows(al, ref_al, C.ALIGN_TOL, label)


def _check_losses(out, ref_losses, ref_sums, label):
    losses, sums = out['losses'].to_host(), out['l1_sums'].to_host()
    e_l = np.abs(losses - ref_losses) / np.abs(ref_losses)
    e_s = np.abs(sums - ref_sums) / np.abs(ref_sums)
    print('{}: losses {} oracle {} (worst {:.3e}), l1_sums worst {:.3e} (bound {:.0e})'.format(
        label, losses, ref_losses, e_l.max(), e_s.max(), C.LOSS_TOL))
    assert np.all(e_l <= C.LOSS_TOL), (losses, ref_losses)
    assert np.all(e_s <= C.LOSS_TOL), (sums, ref_sums)
    assert losses[0] == np.float32(losses[1]) + np.float32(losses[2])


def test_network_evaluate(net):
    """tts_evaluate: T = n_steps * r, the reshapes and the eval_loss strides follow n_mels / reduction."""
    name, hp, eng = net
    ids, mel_t, lin_t, ref = C.network_case(name)
    out = eng.evaluate(ids, mel_t, lin_t, want_sums=True, want_mel=True, want_alignments=True, want_linear=True)
    label = '{} evaluate'.format(name)
    B, S = mel_t.shape[:2]
    assert out['mel'].shape == (B, S * hp.reduction, hp.n_mels)
    assert_parity(out['mel'].to_host(), ref['mel'], BTC, C.FINAL_TOL, label + ' mel')
    assert_alignment_rows(out['alignments'].to_host(), ref['alignments'], C.ALIGN_TOL, label)
    assert_parity(out['linear'].to_host(), ref['linear'], BTC, C.FINAL_TOL, label + ' linear')
    _check_losses(out, ref['losses'], ref['sums'], label)


def test_network_teacher_forced(net):
    name, hp, eng = net
    ids, mel_t, lin_t, ref = C.network_case(name)
    out = eng.teacher_forced(ids, mel_t, lin_t, want_sums=True)
    label = '{} teacher_forced'.format(name)
    assert_parity(out['mel'].to_host(), ref['t_mel'], BTC, C.FINAL_TOL, label + ' mel')
    assert_alignment_rows(out['alignments'].to_host(), ref['t_alignments'], C.ALIGN_TOL, label)
    assert_parity(out['linear'].to_host(), ref['t_linear'], BTC, C.FINAL_TOL, label + ' linear')
    _check_losses(out, ref['t_losses'], ref['t_sums'], label)


def test_network_synthesize_matches_its_stages(net):
    """tts_synthesize against its own stages, bit for bit up to the spectrograms (tests/test_gpu_full_size.py::
    test_end_to_end_synthesize_matches_staged): T, the reshapes and the de-normalising epilogue follow n_mels / reduction.
    The stages themselves are held to the oracle above; the waveform arithmetic is the audio tests' subject."""
    name, hp, eng = net
    ids, _, _, ref = C.network_case(name)
    B, Ts = ids.shape
    S = C.net_shape(hp)[2]
    T, F = S * hp.reduction, 1 + hp.n_fft // 2
    init = np.random.default_rng(1).random((B, F, T)).astype(np.float32)
    out = eng.synthesize(ids, S, 6.02, 99.89, 1.3, 3, WIN, HOP, init_phase=init, peak_normalize=True,
                         want_mel=True, want_alignments=True, want_linear=True)
    mem = eng.encoder_forward(ids)
    mel, al = eng.decoder_forward(mem, S)
    lin = eng.postnet_forward(mel.to_host().reshape(B, T, hp.n_mels))
    mag = eng.denorm_power(lin, 6.02, 99.89, 1.3)
    wav, _ = eng.griffin_lim(mag, 3, WIN, HOP, hp.n_fft, init_phase=init, want_mse=False)
    wav = eng.peak_normalize(wav)
    assert out['wav'].shape == (B, HOP * (T - 1))
    assert np.array_equal(out['mel'].to_host().reshape(B, S, hp.reduction * hp.n_mels), mel.to_host())
    assert np.array_equal(out['linear'].to_host(), lin.to_host())
    assert np.array_equal(out['alignments'].to_host(), al.to_host())
    assert_parity(out['linear'].to_host(), ref['linear'], BTC, C.FINAL_TOL, '{} synthesize linear'.format(name))
    # the fused path de-normalises in the Dense epilogue and peak-normalises in the last iSTFT: equal to rounding
    assert rel_l2(out['wav'].to_host(), wav.to_host()) < 1e-4
    assert np.abs(out['wav'].to_host()).max(axis=1).tolist() == [1.0] * B


def test_teacher_target_stride_beyond_32_bits_is_refused(net):
    """The target's row stride n_steps * r * n_mels is a 32-bit operand of the launch-per-layer decoder GEMM.  Up to n_mels 128
    the limit on n_steps * r (2^24 frames) keeps it there; a wider architecture needs the stride's own check.  The call is
    refused on its arguments: nothing is enqueued (the buffers are dummies)."""
    name, hp, eng = net
    n_steps = (1 << 24) // hp.reduction                   # the largest count the frame limit lets through
    if n_steps * hp.reduction * hp.n_mels <= 0x7FFFFFFF:
        return                                            # (the stride fits at this architecture: nothing to refuse)
    H = pkg('_hip')
    buf = eng.empty((64,))
    for call in (lambda: eng.lib.tts_decoder_forward_teacher(eng.handle, buf.ptr, 1, 1, n_steps, buf.ptr, buf.ptr, None),
                 lambda: eng.lib.tts_teacher_forced(eng.handle, buf.ptr, 1, 1, n_steps, buf.ptr, None, None, None, buf.ptr,
                                                    None, None)):
        assert call() == H.TTS_ERR_INVALID
        assert b'sizes out of range' in eng.lib.tts_last_error(eng.handle)


def test_configurations_beyond_the_limits_are_refused(hparams):
    """tts_create checks the struct before it touches the device: nothing out of range ever reaches a kernel
    (tests/test_architectures_host.py holds the messages; this is the Engine's side of the refusal)."""
    import copy
    sstts = pkg()
    for field, value in [('n_mels', 1040), ('reduction', 1 << 21)]:
        hp = copy.deepcopy(hparams)
        setattr(hp, field, value)
        hp.decoder.target_size = hp.n_mels
        hp.post.projections = ((256, 3, 'relu'), (hp.n_mels, 3, None))
        with pytest.raises(sstts.TtsError) as e:
            sstts.Engine(hp)
        assert e.value.code == -5, (field, str(e.value))


def test_configurations_at_the_limits_are_accepted(hparams):
    """... and the largest accepted n_mels is accepted (a handle without weights: nothing is allocated or run)."""
    import copy
    hp = copy.deepcopy(hparams)
    hp.n_mels = hp.decoder.target_size = 1024
    hp.post.projections = ((256, 3, 'relu'), (1024, 3, None))
    eng = pkg().Engine(hp)
    try:
        assert dict(eng.manifest())['decoder2/decoder/output_projection_wrapper/kernel'] == (256, 5 * 1024)
    finally:
        eng.close()
