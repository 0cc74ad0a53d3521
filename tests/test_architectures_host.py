"""CPU: the bounds of tests/test_gpu_architectures.py are FAIR and have TEETH at every architecture of arch_cases.ARCHS, on
the very inputs the GPU tests use.

(a) fair: the oracle run in float32 -- plain float32 arithmetic of the same operations -- stays within a QUARTER of every
    bound (stage intermediates 1e-4, memory / mel / linear 1e-3, alignment rows 1e-4, losses 1e-5) against its float64 run.  A
    kernel that misses a bound is therefore wrong, not unlucky; an input on which float32 itself came near a bound would show
    up here (the precedent is tests/test_audio_bounds_host.py).
(b) teeth: two deliberately wrong restatements of the decoder (arch_cases.decoder_restated) -- the FIRST frame of the previous
    r-frame group fed back instead of the last, and the last decoder GRU layer's residual connection dropped -- miss the mel
    bound by at least a hundred times at every decoder shape, free-running and teacher-forced.  With r = 1 a group has one
    frame, first and last coincide and the first restatement IS the decoder: that is asserted, and the teeth against a wrong
    frame index come from the architectures with r > 1.
"""
import numpy as np
import pytest

import arch_cases as C
from conftest import pkg
import teacher_oracle as TO
from oracle import tacotron_oracle as O
from parity import BTC, assert_alignment_rows, assert_mel_parity, assert_parity, slice_errors

Q = C.HOST_MARGIN
MEL_AXES = {'utt': 0, 'step': 1, 'col': 2}


def _w32(name):
    return C.arch(name)[1]


@pytest.mark.parametrize('name', list(C.ARCHS))
def test_configure_moves_the_fields_and_keeps_the_manifest_consistent(hparams, name):
    """arch_cases.configure on a copy of the session's hyper-parameters: the base stays untouched, target_size follows n_mels
    and the synthetic weights have the shapes the oracle multiplies."""
    hp = C.configure(hparams, name)
    assert hparams.n_mels == 80 and hparams.reduction == 5 and hparams.decoder.n_gru_layers == 2
    assert hp.decoder.target_size == hp.n_mels
    hp2, w, _ = C.arch(name)
    assert hp2 == hp
    assert w['encoder/embedding'].shape == (hp.vocabulary_size, hp.encoder.embedding_size)
    assert w['decoder2/decoder/output_projection_wrapper/kernel'].shape == (256, hp.n_mels * hp.reduction)


@pytest.mark.parametrize('name', list(C.ARCHS))
def test_float32_encoder_within_a_quarter_of_the_bounds(name):
    hp = C.arch(name)[0]
    for (B, Ts), unknown in [(s, False) for s in C.ENC_SHAPES] + [(C.ENC_SHAPES[1], True)]:
        ids, ref, ref_mem = C.encoder_case(name, B, Ts, unknown)
        got, mem = C.encoder_ref(ids, _w32(name), hp)
        label = 'f32 {} encoder B={} Ts={}{}'.format(name, B, Ts, ' unknown ids' if unknown else '')
        for k in ('prenet', 'bank', 'proj1', 'proj2', 'highway'):
            assert_parity(got[k], ref[k], BTC, Q * C.STAGE_TOL, '{} {}'.format(label, k))
        assert_parity(mem, ref_mem, BTC, Q * C.FINAL_TOL, label + ' memory')
        if unknown:   # the rows of the unknown ids are those of a zero embedding: the first pre-net layer's bias alone
            assert (ids >= hp.vocabulary_size).sum() == 2


@pytest.mark.parametrize('name', list(C.ARCHS))
def test_float32_postnet_within_a_quarter_of_the_bounds(name):
    hp = C.arch(name)[0]
    for B, T in C.POST_SHAPES:
        mel, ref, ref_lin = C.postnet_case(name, B, T)
        got, lin = C.postnet_ref(mel, _w32(name), hp)
        label = 'f32 {} postnet B={} T={}'.format(name, B, T)
        for k in ('bank', 'proj1', 'highway'):
            assert_parity(got[k], ref[k], BTC, Q * C.STAGE_TOL, '{} {}'.format(label, k))
        assert_parity(got['gru'], ref['gru'], BTC, Q * C.FINAL_TOL, label + ' gru')
        assert_parity(lin, ref_lin, BTC, Q * C.FINAL_TOL, label + ' linear')


@pytest.mark.parametrize('B,Ts,S', C.DEC_SHAPES)
@pytest.mark.parametrize('name', list(C.ARCHS))
def test_float32_decoder_within_a_quarter_of_the_bounds(name, B, Ts, S):
    hp = C.arch(name)[0]
    memory, ref_mel, ref_al = C.decoder_case(name, B, Ts, S)
    mel, al = O.decoder(memory, _w32(name), hp, n_steps=S)
    label = 'f32 {} decoder B={} Ts={} S={}'.format(name, B, Ts, S)
    assert_mel_parity(mel, ref_mel, Q * C.FINAL_TOL, label, n_mels=hp.n_mels)
    assert_alignment_rows(al, ref_al, Q * C.ALIGN_TOL, label)
    memory, target, ref_mel, ref_al = C.teacher_case(name, B, Ts, S)
    mel, al = TO.decoder_teacher(memory, target, _w32(name), hp)
    assert_mel_parity(mel, ref_mel, Q * C.FINAL_TOL, label + ' teacher', n_mels=hp.n_mels)
    assert_alignment_rows(al, ref_al, Q * C.ALIGN_TOL, label + ' teacher')


@pytest.mark.parametrize('name', list(C.ARCHS))
def test_float32_network_and_losses_within_a_quarter_of_the_bounds(name):
    hp = C.arch(name)[0]
    ids, mel_t, lin_t, ref = C.network_case(name)
    got = C.network_ref(ids, mel_t, lin_t, _w32(name), hp)
    label = 'f32 {} network'.format(name)
    assert_parity(got['memory'], ref['memory'], BTC, Q * C.FINAL_TOL, label + ' memory')
    for pre in ('', 't_'):
        assert_parity(got[pre + 'mel'], ref[pre + 'mel'], BTC, Q * C.FINAL_TOL, label + ' ' + pre + 'mel')
        assert_alignment_rows(got[pre + 'alignments'], ref[pre + 'alignments'], Q * C.ALIGN_TOL, label + ' ' + pre)
        assert_parity(got[pre + 'linear'], ref[pre + 'linear'], BTC, Q * C.FINAL_TOL, label + ' ' + pre + 'linear')
        for k in ('losses', 'sums'):
            e = np.abs(got[pre + k] - ref[pre + k]) / np.abs(ref[pre + k])
            print('{} {}{}: worst {:.3e} (bound {:.0e})'.format(label, pre, k, e.max(), C.LOSS_TOL))
            assert np.all(e <= Q * C.LOSS_TOL), (pre + k, e)


@pytest.mark.parametrize('name', list(C.ARCHS))
def test_the_restatement_with_its_switches_off_is_the_oracle(name):
    hp, _, w64 = C.arch(name)
    B, Ts, S = C.DEC_SHAPES[1]
    memory, ref_mel, ref_al = C.decoder_case(name, B, Ts, S)
    mel, al = C.decoder_restated(memory.astype(np.float64), w64, hp, S)
    assert np.array_equal(mel, ref_mel) and np.array_equal(al, ref_al)
    memory, target, ref_mel, ref_al = C.teacher_case(name, B, Ts, S)
    mel, al = C.decoder_restated(memory.astype(np.float64), w64, hp, S, target=target.astype(np.float64))
    assert np.array_equal(mel, ref_mel) and np.array_equal(al, ref_al)


def _miss(got, ref):
    """the largest figure assert_mel_parity would hold to the bound on the reduced mel"""
    return max(e for e, _ in slice_errors(got, ref, MEL_AXES).values())


@pytest.mark.parametrize('B,Ts,S', C.DEC_SHAPES)
@pytest.mark.parametrize('name', list(C.ARCHS))
def test_wrong_restatements_miss_the_mel_bound_a_hundredfold(name, B, Ts, S):
    hp, _, w64 = C.arch(name)
    need = C.TEETH * C.FINAL_TOL
    for mode in ('free', 'teacher'):
        if mode == 'free':
            memory, ref_mel, _ = C.decoder_case(name, B, Ts, S)
            target = None
        else:
            memory, target, ref_mel, _ = C.teacher_case(name, B, Ts, S)
            target = target.astype(np.float64)
        m64 = memory.astype(np.float64)
        first = C.decoder_restated(m64, w64, hp, S, target=target, feed='first')[0]
        if hp.reduction == 1:
            assert np.array_equal(first, ref_mel)   # one frame per group: its first frame is its last
        else:
            miss = _miss(first, ref_mel)
            print('{} {} B={} S={} first frame fed: misses by {:.3e}'.format(name, mode, B, S, miss))
            assert miss >= need, (mode, 'first', miss)
        miss = _miss(C.decoder_restated(m64, w64, hp, S, target=target, top_residual=False)[0], ref_mel)
        print('{} {} B={} S={} no top residual: misses by {:.3e}'.format(name, mode, B, S, miss))
        assert miss >= need, (mode, 'residual', miss)


# ---- upper bounds: tts_create checks the struct before it touches the device, so the refusals need no GPU
def _create(**fields):
    import ctypes
    H = pkg('_hip')
    lib = H.load_library()
    cfg = H.TtsConfig()
    lib.tts_default_config(ctypes.byref(cfg))
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(cfg, k)[i] = x
        else:
            setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = lib.tts_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    assert not h.value
    return rc, lib.tts_last_error(None).decode()


@pytest.mark.parametrize('fields,names', [
    (dict(n_mels=1040, post_proj_filters=(256, 1040)), ['n_mels is 1040', 'at most 1024']),
    (dict(vocabulary_size=(1 << 20) + 1), ['1048577', 'at most 1048576']),
    (dict(reduction=1 << 21), ['at most 1048576']),
    (dict(vocabulary_size=1 << 20, embedding_size=1024), ['embedding table', '1073741819']),
    (dict(enc_n_banks=512, enc_n_filters=4096, enc_proj_filters=(256, 128)), ['encoder projection 1', '1073741819']),
    (dict(enc_n_banks=2048, enc_n_filters=8192), ['widest encoder bank', '1073741819']),
    (dict(post_n_banks=1024, post_n_filters=32768), ['widest post-net bank', '1073741819']),
    (dict(post_n_banks=512, post_n_filters=4096), ['post-net projection 1', '1073741819']),
    (dict(n_mels=1024, post_proj_filters=(256, 1024), reduction=16384), ['output projection', '1073741819']),
])
def test_configurations_beyond_the_limits_are_refused_with_the_limit_named(fields, names):
    """n_mels against the 1024-float zero block of the GO frame; every count and width against 2^20; every matrix a GEMM
    loader addresses with 32-bit byte offsets against 2^30 - 5 floats (launch_gemm's own run-time refusal, made at create
    time).  Nothing out of range is ever run."""
    rc, msg = _create(**fields)
    assert rc == pkg('_hip').TTS_ERR_UNSUPPORTED, (rc, msg)
    for n in names:
        assert n in msg, (n, msg)
