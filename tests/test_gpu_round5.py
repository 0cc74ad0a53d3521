"""GPU tests added in round 5 ("Next round" items 5 and 7):

  * the GEMM kernel on inputs that are not kind: sixty decades of dynamic range, float32 denormals, +-Inf / NaN
    (what the exact three-way bf16 split of csrc/gemm_f32.hip does with them is part of the contract now);
  * the post-net at B = 64 x T = 1000 and the whole tts_synthesize at the bench's full size against the ORACLE on
    rows {0, 63} (round 4 compared them at B = 4 / B = 1 and relied on shard invariance for the rest);
  * apply_post_processing = False (reference tacotron/model.py:388-391): final Dense straight on the mel frames;
  * tts_synthesize for another power-of-two n_fft (reference tacotron/params/model.py:13-24 makes it a parameter);
  * a pipelined tts_synthesize with a non-default window / hop (the general Griffin-Lim kernels) beside the persistent decoder;
  * the runnable entry of tacotron/inference.py:130-200 (reads the sentences file, writes {i+1}.wav);
  * the second Griffin-Lim cut of a pipelined call (its last launches on all compute units, option "gl_wide_from")."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG, pkg, rel_l2
import gemm_model
from parity import BTC, assert_alignment_rows, assert_parity
from oracle import audio_oracle as A
from oracle import tacotron_oracle as O

pytestmark = pytest.mark.gpu
N_FFT, WIN, HOP = 2048, 1102, 275
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3


def bench_ids(B, Ts, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, Ts), np.int32)
    for b in range(B):
        L = int(np.clip(round(rng.normal(100, 30)), 20, Ts - 1))
        ids[b, :L] = rng.integers(2, 39, L)
        ids[b, L] = 1
    return ids


def _gemm(engine, x, w, T, ktaps=1, pool=0):
    M, Cin = x.shape
    N = w.shape[0]
    dx, dw = engine.to_device(x), engine.to_device(w)
    dc = engine.empty((M, N))
    engine._check(engine.lib.tts_debug_gemm(engine.handle, dx.data_ptr(), dw.data_ptr(), dc.data_ptr(), M, N, Cin, ktaps, T, pool))
    got = dc.to_host()
    dx.free(); dw.free(); dc.free()
    return got


# ---------------------------------------------------------------------------------------------- GEMM, unkind inputs
def _denormal_terms(v):
    """sum of the magnitudes of the split terms of v that are bf16 DENORMALS (non-zero, below 2^-126), per element"""
    out = np.zeros(v.shape, np.float64)
    for t in gemm_model.split3(v):
        a = np.abs(t.astype(np.float64))
        out += np.where((a > 0) & (a < 2.0 ** -126), a, 0.0)
    return out


@pytest.mark.parametrize('log10_scale_x,log10_scale_w', [(0, 0), (15, -15), (-15, 15), (18, 12), (-18, -12), (-30, 25)])
def test_gemm_over_sixty_decades(engine, log10_scale_x, log10_scale_w):
    """x = hi + mid + lo is exact for every finite float32 whose three terms are bf16 NORMALS; the six products the kernel
    keeps leave a relative error of one f32 rounding of |a| |b|.  The operands here are scaled by 1e-30 ... 1e25 (products
    from 1e-30 to 1e30), each with three decades of spread inside the tile: the scale-free bound of tests/test_gpu_gemm.py
    must hold unchanged -- every element within 4 x the documented arithmetic's own phi (tests/gemm_model.py) on the same
    input, in u = 2^-24 of sum_k |a||w|.

    The split terms stay bf16 normals, asserted here on the host, at every scale but one: at 1e-30 the smallest activations
    (|x| < 2^-102 = 2e-31; they go down to 8e-36) have a denormal lo, some a denormal mid.  Whatever the matrix pipe does
    with such a term (tests below), it is worth less than 2^-126 |w| to an output: exactly that much -- the sum over k of the
    denormal terms' magnitudes times |w| -- is added to the bound there, nowhere else.  It stays under 0.01 u of sum |a||w|."""
    rng = np.random.default_rng(100 + log10_scale_x)
    M, Cin, N = 150, 256, 160
    x = (rng.standard_normal((M, Cin)) * 10.0 ** rng.uniform(-1.5, 1.5, (M, Cin)) * 10.0 ** log10_scale_x).astype(np.float32)
    w = (rng.standard_normal((N, Cin)) * 10.0 ** rng.uniform(-1.5, 1.5, (N, Cin)) * 10.0 ** log10_scale_w).astype(np.float32)
    ref, D = gemm_model.reference(x, w, 1, 50, 0)
    assert np.isfinite(ref).all() and np.abs(ref).max() < 1e37
    den_x, den_w = _denormal_terms(x), _denormal_terms(w)
    assert not den_w.any() and np.abs(x).min() >= 2.0 ** -126 and np.abs(w).min() >= 2.0 ** -102
    if log10_scale_x != -30:
        assert not den_x.any() and np.abs(x).min() >= 2.0 ** -102
    flushed = den_x @ np.abs(w.astype(np.float64)).T
    assert (flushed <= 1e-2 * gemm_model.U * D).all()
    p_model = gemm_model.phi(gemm_model.model_conv(x, w, 1, 50, 0), ref, D)
    got = _gemm(engine, x, w, T=50)
    assert np.isfinite(got).all()
    excess = (np.abs(got.astype(np.float64) - ref) - flushed) / D / gemm_model.U
    e = rel_l2(got, ref)
    print('gemm scales 1e{} x 1e{}: phi GPU {:.3f} u (less the denormal terms: {:.3f} u), model {:.3f} u, rel-L2 {:.2e}'.format(
        log10_scale_x, log10_scale_w, gemm_model.phi(got, ref, D), excess.max(), p_model, e))
    assert excess.max() <= 4 * p_model, (excess.max(), p_model)


def test_gemm_denormal_operands(engine):
    """Operands down in the float32 denormal range (|x| < 1.18e-38): hi, mid and lo are then bf16 denormals as well.  The
    matrix pipe flushes them or it does not -- either way the result may only differ from the exact one by what the
    flushed terms are worth: an ABSOLUTE error below K * 2^-126 * max|w| per output (here 1.5e-36), far below anything a
    float32 network value resolves.  Documented, not exact: csrc/gemm_f32.hip."""
    rng = np.random.default_rng(5)
    M, Cin, N = 128, 128, 128
    x = (rng.standard_normal((M, Cin)) * 1e-39).astype(np.float32)       # denormals
    x[::2] = (rng.standard_normal((M // 2, Cin)) * 1e-36).astype(np.float32)   # ... next to small normals whose lo terms are denormal
    w = rng.standard_normal((N, Cin)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    got = _gemm(engine, x, w, T=M)
    err = np.abs(got.astype(np.float64) - ref).max()
    print('gemm denormal operands: max abs error {:.2e} (result scale {:.2e})'.format(err, np.abs(ref).max()))
    assert np.isfinite(got).all()
    assert err < Cin * 2.0 ** -126 * np.abs(w).max() * 4


def test_gemm_nonfinite_operands_stay_nonfinite(engine):
    """+-Inf and NaN: the split of an infinity is (Inf, NaN, NaN) -- Inf - Inf in the first subtraction -- so a row or
    column that holds an Inf or a NaN comes out as NaN where the f32-input MFMA (-DGEMM_F32_MFMA) would give +-Inf for a
    lone infinity.  The contract: a non-finite operand makes every output that depends on it NON-FINITE (never a finite
    number), and every output that does not depend on it stays exact."""
    rng = np.random.default_rng(9)
    M, Cin, N = 128, 128, 128
    x = rng.standard_normal((M, Cin)).astype(np.float32)
    w = (rng.standard_normal((N, Cin)) * 0.05).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    x[3, 17] = np.inf
    x[40, 0] = -np.inf
    x[77, 100] = np.nan
    w[5, 64] = np.inf
    got = _gemm(engine, x, w, T=M)
    bad_rows, bad_cols = [3, 40, 77], [5]
    assert not np.isfinite(got[bad_rows]).any()
    assert not np.isfinite(got[:, bad_cols]).any()
    ok = np.ones((M, N), bool)
    ok[bad_rows] = False
    ok[:, bad_cols] = False
    assert np.isfinite(got[ok]).all()
    assert rel_l2(got[ok], ref[ok]) < 1e-5


# ---------------------------------------------------------------------------------------------- full size vs the oracle
def test_postnet_b64_t1000_vs_oracle_rows_0_and_63(engine, hparams, weights64):
    """Config 4's network half at its full size, first and last row of the batch against the oracle (the rows in
    between rest on tests/test_gpu_full_size.py::test_shard_invariance)."""
    rng = np.random.default_rng(11)
    mel = rng.random((64, 1000, 80)).astype(np.float32)
    got = engine.postnet_forward(engine.to_device(mel)).to_host()
    assert got.shape == (64, 1000, 1025) and np.isfinite(got).all()
    for b in (0, 63):
        ref = O.post_process(mel[b:b + 1].astype(np.float64), weights64, hparams)
        e = rel_l2(got[b:b + 1], ref)
        print('post-net B=64 T=1000 row {}: rel-L2 {:.3e}'.format(b, e))
        assert e < 1e-3
        assert_parity(got[b:b + 1], ref, BTC, 1e-3, 'post-net B=64 T=1000 row {} linear'.format(b))


def test_synthesize_b64_full_size_vs_oracle_rows_0_and_63(engine, hparams, weights64):
    """The bench's call -- 64 utterances, T_sent 150, 200 decoder steps, 60 Griffin-Lim iterations -- through
    tts_synthesize (pipelined: the second call of the shape, with the persistent decoder), rows 0 and 63 against the
    oracle: mel and linear spectrograms rel-L2 <= 1e-3, alignments max-abs <= 1e-4, and the waveform through the
    spectral convergence of 60 iterations from identical initial phases (within 1 % of the oracle's)."""
    ids = bench_ids(64, 150, 1234)
    rng = np.random.default_rng(42)
    init = rng.random((64, 1025, 1000), dtype=np.float32)
    d_ids, d_init = engine.to_device(ids), engine.to_device(init)
    kw = dict(n_steps=200, ref_db=REF_DB, max_db=MAX_DB, power=POWER, n_iter=60, win_length=WIN, hop_length=HOP,
              init_phase=d_init, peak_normalize=False, want_mel=True, want_linear=True, want_alignments=True)
    engine.synthesize(d_ids, **kw)            # the first call of a shape runs unpipelined
    out = engine.synthesize(d_ids, **kw)      # pipelined: persistent decoder beside the first call's Griffin-Lim
    engine.synchronize()
    mel, lin, al, wav = (out[k].to_host() for k in ('mel', 'linear', 'alignments', 'wav'))
    assert mel.shape == (64, 1000, 80) and lin.shape == (64, 1000, 1025) and wav.shape == (64, HOP * 999)
    assert np.isfinite(wav).all()
    for b in (0, 63):
        ref = O.tacotron_predict(ids[b:b + 1], weights64, hparams, n_steps=200)
        e_mel, e_lin = rel_l2(mel[b:b + 1], ref['mel']), rel_l2(lin[b:b + 1], ref['linear'])
        e_al = float(np.abs(al[:, b:b + 1] - ref['alignments']).max())
        mag_pow = A.linear_to_magnitude(ref['linear'][0].astype(np.float32), REF_DB, MAX_DB, POWER)
        ref_wav, ref_mse = A.griffin_lim_v2(mag_pow, WIN, HOP, N_FFT, 60, init_phase=init[b])
        est_ref = np.abs(A.stft(np.asarray(ref_wav, np.float32), N_FFT, HOP, WIN)).astype(np.float64)
        est_hip = np.abs(A.stft(wav[b], N_FFT, HOP, WIN)).astype(np.float64)
        sc_ref = float(np.linalg.norm(est_ref - mag_pow) / np.linalg.norm(mag_pow))
        sc_hip = float(np.linalg.norm(est_hip - mag_pow) / np.linalg.norm(mag_pow))
        print('synthesize B=64 row {}: mel {:.2e} linear {:.2e} align {:.2e}; spectral convergence {:.5f} vs oracle {:.5f}'.format(
            b, e_mel, e_lin, e_al, sc_hip, sc_ref))
        assert e_mel < 1e-3 and e_lin < 1e-3 and e_al < 1e-4
        assert abs(sc_hip - sc_ref) <= 0.01 * sc_ref
        label = 'synthesize B=64 row {}'.format(b)
        assert_parity(mel[b:b + 1], ref['mel'], BTC, 1e-3, label + ' mel')
        assert_parity(lin[b:b + 1], ref['linear'], BTC, 1e-3, label + ' linear')
        assert_alignment_rows(al[:, b:b + 1], ref['alignments'], 1e-4, label)


# ---------------------------------------------------------------------------------------------- functional corners
@pytest.fixture(scope='module')
def no_post(hparams):
    hp = copy.deepcopy(hparams)
    hp.apply_post_processing = False
    W = pkg('tacotron.weights')
    w = W.synthetic_weights(3, hp)
    eng = pkg().Engine(hp)
    eng.load_weights(w)
    yield hp, w, eng
    eng.close()


def test_without_post_processing_manifest(no_post):
    hp, w, eng = no_post
    names = dict(eng.manifest())
    assert set(names) == set(w)
    assert not any(n.startswith('post_process/') for n in names)
    assert tuple(names['dense/kernel']) == (80, 1025) == w['dense/kernel'].shape


@pytest.mark.parametrize('B,Ts,S', [(2, 9, 4), (5, 33, 7)])
def test_without_post_processing_vs_oracle(no_post, B, Ts, S):
    """reference tacotron/model.py:388-398 with apply_post_processing=False: output_linear_spec = Dense(1025)(output_mel_spec)."""
    hp, w, eng = no_post
    rng = np.random.default_rng(B)
    ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
    ids[:, -1] = 1
    ref = O.tacotron_predict(ids, O.cast_weights(w, np.float64), hp, n_steps=S)
    init = rng.random((B, 1025, 5 * S)).astype(np.float32)
    out = eng.synthesize(ids, S, REF_DB, MAX_DB, POWER, 2, WIN, HOP, init_phase=init, peak_normalize=False,
                         want_mel=True, want_linear=True)
    lin_staged = eng.postnet_forward(out['mel'].to_host())
    e_mel, e_lin = rel_l2(out['mel'].to_host(), ref['mel']), rel_l2(out['linear'].to_host(), ref['linear'])
    print('apply_post_processing=False B={} Ts={} S={}: mel {:.2e} linear {:.2e}'.format(B, Ts, S, e_mel, e_lin))
    assert e_mel < 1e-3 and e_lin < 1e-3
    label = 'apply_post_processing=False B={} Ts={} S={}'.format(B, Ts, S)
    assert_parity(out['mel'].to_host(), ref['mel'], BTC, 1e-3, label + ' mel')
    assert_parity(out['linear'].to_host(), ref['linear'], BTC, 1e-3, label + ' linear')
    assert np.array_equal(lin_staged.to_host(), out['linear'].to_host())
    for b in range(B):
        mag = A.linear_to_magnitude(ref['linear'][b].astype(np.float32), REF_DB, MAX_DB, POWER)
        wav_ref = A.spectrogram_to_wav(mag, WIN, HOP, N_FFT, 2, init_phase=init[b])
        assert rel_l2(out['wav'].to_host()[b], wav_ref) < 1e-3
    # the facade takes the flag from the hyper-parameters (round 4 raised NotImplementedError here)
    T = pkg('tacotron.model')
    model = T.Tacotron(inputs=T.Tacotron.model_placeholders(), mode=T.Mode.PREDICT, engine=eng, hparams=hp)
    pred = model.predict_device(ids, n_steps=S)
    assert np.array_equal(pred['linear'].to_host(), out['linear'].to_host())


@pytest.mark.parametrize('n_fft,win,hop', [(1024, 800, 200), (512, 512, 128)])
def test_synthesize_with_another_n_fft(hparams, n_fft, win, hop):
    """n_fft is a model parameter (reference tacotron/params/model.py:13-24): the final Dense then has 1 + n_fft / 2
    outputs and Griffin-Lim runs in the general kernels.  End to end against the oracle (round 4: TTS_ERR_UNSUPPORTED)."""
    hp = copy.deepcopy(hparams)
    hp.n_fft = n_fft
    W = pkg('tacotron.weights')
    w = W.synthetic_weights(4, hp)
    F = 1 + n_fft // 2
    assert w['dense/kernel'].shape == (256, F)
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        rng = np.random.default_rng(n_fft)
        B, Ts, S = 3, 17, 8
        ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
        ids[:, -1] = 1
        T = 5 * S
        init = rng.random((B, F, T)).astype(np.float32)
        out = eng.synthesize(ids, S, REF_DB, MAX_DB, POWER, 3, win, hop, init_phase=init, peak_normalize=False,
                             want_mel=True, want_linear=True)
        ref = O.tacotron_predict(ids, O.cast_weights(w, np.float64), hp, n_steps=S)
        lin = out['linear'].to_host()
        assert lin.shape == (B, T, F)
        e_lin = rel_l2(lin, ref['linear'])
        errs = []
        for b in range(B):
            mag = A.linear_to_magnitude(ref['linear'][b].astype(np.float32), REF_DB, MAX_DB, POWER)
            wav_ref = A.spectrogram_to_wav(mag, win, hop, n_fft, 3, init_phase=init[b])
            errs.append(rel_l2(out['wav'].to_host()[b], wav_ref))
        print('synthesize n_fft={} win={} hop={}: linear {:.2e}, wav {}'.format(n_fft, win, hop, e_lin, ['%.2e' % e for e in errs]))
        assert e_lin < 1e-3 and max(errs) < 1e-3
    finally:
        eng.close()


def test_pipelined_synthesize_with_the_general_griffin_lim_kernels(engine):
    """A window / hop pair the streaming kernel does not cover (win 1200 / hop 300 at n_fft 2048) runs Griffin-Lim in the
    general kernels: full grids of short workgroups on the main stream while the NEXT call's persistent decoder claims its
    compute units on the front stream.  Pipelined calls must equal serial calls bit for bit."""
    batches = [bench_ids(6, 25, 300 + i) for i in range(5)]

    def run(pipeline):
        engine.set_option('pipeline', pipeline)
        dev = [engine.to_device(b) for b in batches]
        outs = [engine.synthesize(d, 8, REF_DB, MAX_DB, POWER, 4, 1200, 300, seed=40 + i, want_mel=True, want_linear=True)
                for i, d in enumerate(dev)]
        engine.synchronize()
        return [{k: v.to_host() for k, v in o.items() if v is not None} for o in outs]

    try:
        engine.set_option('persistent_decoder', 2)
        run(1)   # shapes known
        seq = run(0)
        pip = run(1)
        for i, (a, b) in enumerate(zip(seq, pip)):
            assert np.isfinite(a['wav']).all() and np.abs(a['wav']).max() > 0
            for k in a:
                assert np.array_equal(a[k], b[k]), (i, k)
    finally:
        engine.set_option('pipeline', 1)
        engine.set_option('persistent_decoder', 1)


def test_synthesize_at_the_16_khz_window_runs_the_streaming_kernel(engine, weights64, hparams):
    """win 800 / hop 200 (the reference's 50 ms / 12.5 ms at a 16 kHz sampling rate, audio/conversion.py:122-136) at the model's
    n_fft: tts_synthesize reconstructs in the streaming kernel's second instantiation (round 6) -- same stages, same seeded
    start -- and its waveform equals the staged path's (tts_griffin_lim on the de-normalised spectrogram: same kernel, same
    cut) to rounding, the oracle's within the bounds of the 1102 / 275 tests."""
    ids = bench_ids(3, 30, 21)
    S, n_iter, win, hop = 12, 5, 800, 200
    T = S * hparams.reduction
    init = np.random.default_rng(16).random((3, 1025, T)).astype(np.float32)
    out = engine.synthesize(ids, S, REF_DB, MAX_DB, POWER, n_iter, win, hop, init_phase=init, peak_normalize=True, want_mel=True,
                            want_linear=True)
    wav = out['wav'].to_host()
    lin = out['linear'].to_host()
    for b in range(3):
        mag = A.linear_to_magnitude(lin[b], REF_DB, MAX_DB, POWER)
        ref = A.peak_normalize(A.spectrogram_to_wav(mag, win, hop, 2048, n_iter, init_phase=init[b]))
        assert ref.shape == wav[b].shape == (hop * (T - 1),)
        assert rel_l2(wav[b], ref) < 1e-4 * n_iter, b
    assert np.isfinite(wav).all() and np.abs(wav).max() > 0


@pytest.mark.parametrize('peak', [True, False])
def test_wide_last_griffin_lim_launches(engine, peak):
    """Option "gl_wide_from" (api_pipeline.hip, gl_wide_from()): the launches of a pipelined call from that index on are cut for all
    compute units instead of all but `reserve_cus`.  Another overlap-add order, so: equal to the one-cut form to the
    reconstruction's own rounding, bit-identical call after call, and the peak normalisation / the sample count intact."""
    B, S, n_iter = 24, 60, 12   # 300 frames, four launches of three iterations and the final one
    batches = [bench_ids(B, 120, 500 + i) for i in range(3)]

    def run(wide):
        engine.set_option('gl_wide_from', wide)
        dev = [engine.to_device(b) for b in batches]
        outs = [engine.synthesize(d, S, REF_DB, MAX_DB, POWER, n_iter, WIN, HOP, seed=7 + i, peak_normalize=peak)
                for i, d in enumerate(dev)]
        engine.synchronize()
        return [o['wav'].to_host() for o in outs]

    try:
        engine.set_option('pipeline', 1)
        run(-2)   # shapes known: the calls below are pipelined from the first one
        one_cut = run(-2)
        for wide in (0, 2, 4):   # every launch, the last two and the final one, the final one alone
            a = run(wide)
            b = run(wide)
            for i in range(len(batches)):
                assert np.array_equal(a[i], b[i]), (wide, i)
                assert np.isfinite(a[i]).all()
                for r in range(B):
                    assert rel_l2(a[i][r], one_cut[i][r]) < 1e-4 * n_iter, (wide, i, r)
                if peak:
                    assert np.allclose(np.abs(a[i]).max(axis=1), 1.0, atol=1e-6)
    finally:
        engine.set_option('gl_wide_from', -1)


def test_wide_launches_between_calls_of_other_shapes(engine):
    """The decoder of a call waits for the post-net of the call before it when the call two back ended its Griffin-Lim phase
    in wide launches (api_pipeline.hip, gl_wide_used): calls of two shapes alternate here, so the gate, the two cuts and the
    workspaces of both shapes meet in one sequence.  Bit-identical run to run, equal to the one-cut form to rounding."""
    shapes = [(24, 60), (6, 30), (24, 60), (6, 30), (24, 60), (24, 60)]
    batches = [bench_ids(B, 100, 700 + i) for i, (B, _) in enumerate(shapes)]

    def run(wide):
        engine.set_option('gl_wide_from', wide)
        dev = [engine.to_device(b) for b in batches]
        outs = [engine.synthesize(d, S, REF_DB, MAX_DB, POWER, 9, WIN, HOP, seed=3 + i, want_mel=True)
                for i, (d, (_, S)) in enumerate(zip(dev, shapes))]
        engine.synchronize()
        return [(o['wav'].to_host(), o['mel'].to_host()) for o in outs]

    try:
        engine.set_option('pipeline', 1)
        run(-2)
        one_cut = run(-2)
        a = run(1)
        b = run(1)
        for i in range(len(shapes)):
            assert np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]), i
            assert np.array_equal(a[i][1], one_cut[i][1]), i   # the network's output does not depend on the cut
            for r in range(shapes[i][0]):
                assert rel_l2(a[i][0][r], one_cut[i][0][r]) < 1e-4 * 9, (i, r)
    finally:
        engine.set_option('gl_wide_from', -1)


def test_inference_main_reads_the_sentences_file(weights, tmp_path):
    """reference tacotron/inference.py:130-200 as a runnable entry: sentences file in, {i+1}.wav out (one per line, in order)."""
    I = pkg('tacotron.inference')
    P = pkg('tacotron.params')
    sent = tmp_path / 'sentences.txt'
    sent.write_text('Hello world.\nMr. Smith said hi!\nOne more.\n')
    out = tmp_path / 'out'
    out.mkdir()
    np.savez(tmp_path / 'weights.npz', **weights)
    P.model_params.decoder.maximum_iterations = 20       # 4 decoder steps keep the test small
    P.model_params.reconstruction_iterations = 2
    try:
        with pytest.raises(NotADirectoryError):
            I.main(['--synthesis-file', str(sent), '--synthesis-dir', str(tmp_path / 'missing'), '--weights', str(tmp_path / 'weights.npz')])
        assert I.main(['--synthesis-file', str(sent), '--synthesis-dir', str(out), '--weights', str(tmp_path / 'weights.npz')]) == 0
    finally:
        P.model_params.decoder.maximum_iterations = 1000
        P.model_params.reconstruction_iterations = 50
    assert sorted(os.listdir(out)) == ['1.wav', '2.wav', '3.wav']
    from scipy.io import wavfile
    sr, d = wavfile.read(out / '3.wav')
    assert sr == 22050 and d.dtype == np.float32 and d.shape == (275 * 19,) and np.isclose(np.abs(d).max(), 1.0)
    # ... and as `python -m <package>.tacotron.inference` (argument parsing only: no second process on the GPU)
    r = subprocess.run([sys.executable, '-m', PKG + '.tacotron.inference', '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b'--synthesis-file' in r.stdout, r.stderr.decode()[-500:]
