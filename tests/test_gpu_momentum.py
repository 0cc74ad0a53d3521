"""GPU: fast Griffin-Lim (the handle option "gl_momentum", include/sstts_hip.h) through the C ABI.

The bound is the project's own for Griffin-Lim -- 1e-4 n_iter per utterance and per hop segment, 1e-3 relative on the mse
-- against the float64 restatement of momentum_oracle.py; test_momentum_host.py shows a float32 restatement within a
quarter of it on the same inputs.  Everything else is bits: the cut into runs, the utterance's place in a batch, the
option's default, its refusal of bad values, tts_synthesize against its stages.  Every test here that sets "gl_momentum"
fails on a library without the option, which refuses the key.
"""
import numpy as np
import pytest

import audio_cases as C
import momentum_oracle as M
from conftest import pkg, rel_l2
from parity import assert_segment_parity
from test_gpu_audio import seed_u
from test_gpu_neighbours import neighbour  # noqa: F401  (the fixture: a second handle that keeps GEMM waves on the chip)

pytestmark = pytest.mark.gpu
N_FFT, WIN, HOP = 2048, 1102, 275
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gl(engine, mag, n_iter, win=WIN, hop=HOP, n_fft=N_FFT, init=None, seed=0, want_mse=True, **options):
    """tts_griffin_lim under handle options that are put back afterwards -> (waveform, mse or None) on the host"""
    restore = {'gl_momentum': 0, 'gl_pair': 3, 'gl_run_len': 0, 'gl_runs': 0, 'debug_hooks': 0}
    order = sorted(options, key=lambda k: k != 'debug_hooks')          # the hooks' switch first
    try:
        for k in order:
            engine.set_option(k, options[k])
        wav, mse = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=init, seed=seed, want_mse=want_mse)
        return wav.to_host(), (mse.to_host() if want_mse else None)
    finally:
        for k in sorted(options, key=lambda k: k == 'debug_hooks'):    # ... and last
            engine.set_option(k, restore[k])


def _against_restatement(engine, key, case, label, want_mse=True, **options):
    mag, init, win, hop, n_fft, n_iter, momentum = case
    wav, mse = _gl(engine, mag, n_iter, win, hop, n_fft, init=init, want_mse=want_mse,
                   gl_momentum=int(round(momentum * 1000)), **options)
    for b, (ref_wav, ref_mse) in enumerate(M.reference(key, case)):
        assert wav[b].shape == ref_wav.shape
        assert_segment_parity(wav[b], ref_wav, hop, C.gl_tol(n_iter), '{} b={}'.format(label, b))
        if want_mse:
            print('{} b={}: mse {} vs {}'.format(label, b, mse[b], ref_mse))
            assert abs(mse[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9


# ---------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize('per_launch', [1, 2, 3])
@pytest.mark.parametrize('k', range(len(C.GL_PER_LAUNCH)))
def test_momentum_streaming_kernel(engine, k, per_launch):
    """1102 / 275 at alpha = 0.99 under every "gl_pair": a momentum call runs one iteration per launch whatever the
    option says, with and without the mse form, runs shorter than the lead (T = 9) and several laps of the ring (T = 151)"""
    _against_restatement(engine, ('per_launch', k, 0.99), M.case_per_launch(k, 0.99),
                         'momentum 0.99 gl_pair {} {}'.format(per_launch, C.GL_PER_LAUNCH[k]),
                         want_mse=C.GL_PER_LAUNCH[k][3], gl_pair=per_launch)


@pytest.mark.parametrize('k', range(len(C.GL_PER_LAUNCH)))
def test_momentum_streaming_kernel_half(engine, k):
    _against_restatement(engine, ('per_launch', k, 0.5), M.case_per_launch(k, 0.5),
                         'momentum 0.5 {}'.format(C.GL_PER_LAUNCH[k]), want_mse=C.GL_PER_LAUNCH[k][3])


@pytest.mark.parametrize('per_launch', [1, 3])
def test_momentum_streaming_kernel_second_window(engine, per_launch):
    """the 800 / 200 instantiation, 7 iterations, the inputs of the plain test of that window"""
    _against_restatement(engine, ('second_window', per_launch), M.case_second_window(per_launch),
                         'momentum 800/200 input {}'.format(per_launch))


@pytest.mark.parametrize('k', range(5))
def test_momentum_general_kernels(engine, k):
    """glg_stft_kernel: four other transform sizes and the model's with another window, 3 iterations"""
    _against_restatement(engine, ('other_sizes', k), M.case_other_sizes(k), 'momentum general {}'.format(C.GL_OTHER_SIZES[k]))


# ---------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize('run_len', [8, 104])
@pytest.mark.parametrize('per_launch,n_iter,want_mse', C.GL_RUN_CUT_FORMS)
def test_momentum_bits_do_not_depend_on_the_cut_or_the_batch(engine, run_len, per_launch, n_iter, want_mse):
    """Runs of one round of the waves and runs of 104 frames against the planner's cut: the same bits of waveform and
    mse (a run reads and writes the previous projection of exactly the frames it owns); utterance 0 alone: the bits it
    has inside the batch of five.  The four-iteration form also against the restatement."""
    mag, init = C.gl_run_cut_input(run_len)
    whole_w, whole_m = _gl(engine, mag, n_iter, init=init, want_mse=want_mse, gl_momentum=990, gl_pair=per_launch)
    cut_w, cut_m = _gl(engine, mag, n_iter, init=init, want_mse=want_mse, gl_momentum=990, gl_pair=per_launch,
                       debug_hooks=1, gl_run_len=run_len)
    one_w, one_m = _gl(engine, mag[:1], n_iter, init=init[:1], want_mse=want_mse, gl_momentum=990, gl_pair=per_launch)
    plain_w, _ = _gl(engine, mag, n_iter, init=init, want_mse=want_mse, gl_pair=per_launch)
    assert np.isfinite(whole_w).all() and not np.array_equal(whole_w, plain_w)
    assert np.array_equal(_bits(cut_w), _bits(whole_w))
    assert np.array_equal(_bits(one_w[0]), _bits(whole_w[0]))
    if want_mse:
        assert np.array_equal(_bits(cut_m), _bits(whole_m)) and _bits(one_m)[0] == _bits(whole_m)[0]
    if n_iter == 4:
        for b, (ref_wav, _) in enumerate(M.reference(('run_cut', run_len), M.case_run_cut(run_len))):
            assert_segment_parity(cut_w[b], ref_wav, HOP, C.gl_tol(n_iter), 'momentum run_len {} b={}'.format(run_len, b))


@pytest.mark.parametrize('n_iter,want_mse', [(2, False), (4, True), (7, False)])
@pytest.mark.parametrize('seed', [0, (7 << 32) + 12345])
def test_momentum_seeded_start(engine, n_iter, want_mse, seed):
    """init_phase NULL: the first launch draws the phasors itself (the SEEDED momentum instantiations, whose first
    iteration also has no previous projection).  Run to run the same bits; against the restatement started from the numpy
    restatement of the draws, per utterance within the Griffin-Lim bound, as test_gpu_audio.py holds the plain seeded start."""
    B, T = 3, 41
    mag = C.synth_mag(np.random.default_rng(77), B, T)
    u = seed_u(seed, B, mag.shape[1], T)
    w_seed, m_seed = _gl(engine, mag, n_iter, seed=seed, want_mse=want_mse, gl_momentum=990)
    w_again, _ = _gl(engine, mag, n_iter, seed=seed, want_mse=want_mse, gl_momentum=990)
    w_expl, _ = _gl(engine, mag, n_iter, init=u, want_mse=want_mse, gl_momentum=990)
    w_plain, _ = _gl(engine, mag, n_iter, seed=seed, want_mse=want_mse)
    assert np.array_equal(_bits(w_seed), _bits(w_again))
    assert not np.array_equal(w_seed, w_plain)
    for b in range(B):
        ref_wav, ref_mse = M.griffin_lim_momentum(mag[b], WIN, HOP, N_FFT, n_iter, u[b], 0.99)
        e, e_expl, e_pair = rel_l2(w_seed[b], ref_wav), rel_l2(w_expl[b], ref_wav), rel_l2(w_seed[b], w_expl[b])
        print('momentum seeded it={} seed={} b={}: rel-L2 seeded {:.3e}, explicit array {:.3e}, one against the other {:.3e}'.format(
            n_iter, seed, b, e, e_expl, e_pair))
        # the in-kernel draw and the same numbers as an explicit array: each within the Griffin-Lim bound of the restatement
        # started from them, so within twice the bound of each other (the draws are the same phasors)
        assert e < C.gl_tol(n_iter) and e_expl < C.gl_tol(n_iter)
        assert e_pair < 2 * C.gl_tol(n_iter)
        if want_mse:
            assert abs(m_seed[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9


def test_momentum_option_default_refusals_and_stickiness(engine, hparams, weights):
    """0 set explicitly: the bits of a handle that never heard of the option; -1 and 1000: TTS_ERR_INVALID, the option
    stays what it was; 990 -> call -> 0 -> call: the first plain call's bits again."""
    mag, init = C.gl_per_launch_input(2, 40, 6)
    fresh = pkg().Engine(hparams)
    try:
        fresh.load_weights(weights)
        f_wav, f_mse = fresh.griffin_lim(mag, 6, WIN, HOP, N_FFT, init_phase=init)
        f_wav, f_mse = f_wav.to_host(), f_mse.to_host()
    finally:
        fresh.close()
    lib, h = engine.lib, engine.handle

    def call():
        wav, mse = engine.griffin_lim(mag, 6, WIN, HOP, N_FFT, init_phase=init)
        return wav.to_host(), mse.to_host()

    try:
        engine.set_option('gl_momentum', 0)
        p_wav, p_mse = call()
        assert np.array_equal(_bits(p_wav), _bits(f_wav)) and np.array_equal(_bits(p_mse), _bits(f_mse))
        engine.set_option('gl_momentum', 990)
        m_wav, m_mse = call()
        assert not np.array_equal(m_wav, p_wav)
        for bad in (-1, 1000):
            assert lib.tts_set_option(h, b'gl_momentum', bad) == -1          # TTS_ERR_INVALID
            assert b'gl_momentum' in lib.tts_last_error(h)
            w, m = call()
            assert np.array_equal(_bits(w), _bits(m_wav)) and np.array_equal(_bits(m), _bits(m_mse)), bad
        engine.set_option('gl_momentum', 0)
        for bad in (-1, 1000):
            assert lib.tts_set_option(h, b'gl_momentum', bad) == -1
        w, m = call()
        assert np.array_equal(_bits(w), _bits(p_wav)) and np.array_equal(_bits(m), _bits(p_mse))
        # the keyword of the Python engine: set for the call, put back afterwards
        wav, _ = engine.griffin_lim(mag, 6, WIN, HOP, N_FFT, init_phase=init, momentum=0.99)
        assert np.array_equal(_bits(wav.to_host()), _bits(m_wav)) and engine._gl_momentum == 0
        w, _ = call()
        assert np.array_equal(_bits(w), _bits(p_wav))
    finally:
        engine.set_option('gl_momentum', 0)


def _ids(B, Ts, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
    ids[:, -1] = 1
    return ids


def test_momentum_synthesize_equals_its_stages(engine, hparams):
    """tts_synthesize under the option = encoder -> decoder -> post-net -> tts_denorm_power -> tts_griffin_lim under the
    option, bit for bit: they share the internal Griffin-Lim routine."""
    B, Ts, S, n_iter = 2, 13, 4, 5
    T = S * hparams.reduction
    ids = _ids(B, Ts, 0)
    init = np.random.default_rng(1).random((B, 1025, T)).astype(np.float32)
    try:
        engine.set_option('gl_momentum', 990)
        out = engine.synthesize(ids, S, REF_DB, MAX_DB, POWER, n_iter, WIN, HOP, init_phase=init, peak_normalize=False,
                                want_mel=True, want_linear=True)
        wav = out['wav'].to_host()
        memory = engine.encoder_forward(ids)
        mel, _ = engine.decoder_forward(memory, S)
        assert np.array_equal(_bits(mel.to_host()).reshape(-1), _bits(out['mel'].to_host()).reshape(-1))
        lin = engine.postnet_forward(mel.to_host().reshape(B, T, hparams.n_mels))
        assert np.array_equal(_bits(lin.to_host()), _bits(out['linear'].to_host()))
        mag = engine.denorm_power(lin, REF_DB, MAX_DB, POWER)
        staged, _ = engine.griffin_lim(mag, n_iter, WIN, HOP, N_FFT, init_phase=init, want_mse=False)
        staged = staged.to_host()
        engine.set_option('gl_momentum', 0)
        plain = engine.synthesize(ids, S, REF_DB, MAX_DB, POWER, n_iter, WIN, HOP, init_phase=init, peak_normalize=False)
        plain = plain['wav'].to_host()
    finally:
        engine.set_option('gl_momentum', 0)
    assert np.isfinite(wav).all() and np.abs(wav).max() > 0
    assert not np.array_equal(wav, plain)
    assert np.array_equal(_bits(wav), _bits(staged))


def test_momentum_three_host_calls_in_flight_equal_serial_calls(engine, hparams):
    """tts_synthesize_host, three calls in flight under the option (the option is read when a call is made) =
    tts_synthesize + copy, one call at a time"""
    B, Ts, S, n_iter = 2, 13, 4, 5
    batches = [_ids(B, Ts, 20 + k) for k in range(4)]
    args = (S, REF_DB, MAX_DB, POWER, n_iter, WIN, HOP)
    reset = np.full((3, 5), 2, np.int32)   # a call of another shape: both sequences then start unpipelined
    try:
        engine.set_option('gl_momentum', 990)
        engine.synthesize(reset, *args, seed=1)
        got, pending = [], []
        for k, ids in enumerate(batches):
            pending.append(engine.synthesize_host(ids, *args, seed=50 + k, peak_normalize=True))
            if len(pending) == 3:
                got.append(engine.wait_host(pending.pop(0)))
        while pending:
            got.append(engine.wait_host(pending.pop(0)))
        engine.synthesize(reset, *args, seed=1)
        want = []
        for k, ids in enumerate(batches):
            want.append(engine.synthesize(engine.to_device(ids), *args, seed=50 + k, peak_normalize=True)['wav'].to_host())
        engine.set_option('gl_momentum', 0)
        plain = engine.synthesize(engine.to_device(batches[0]), *args, seed=50, peak_normalize=True)['wav'].to_host()
    finally:
        engine.set_option('gl_momentum', 0)
    assert not np.array_equal(want[0], plain)
    for k in range(len(batches)):
        assert np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize('win,hop', [(1102, 275), (1200, 300)], ids=['streaming', 'general'])
def test_momentum_switched_on_between_pipelined_calls(hparams, weights, win, hop):
    """The option set between two pipelined tts_synthesize calls of one shape, on a handle that has never had momentum: the
    buffer of the previous projection gets its first allocation in that call, which therefore runs unpipelined like the
    first call of a shape.  Calls made back to back = the same calls each waited for, bit for bit."""
    B, Ts, S, n_iter = 2, 13, 6, 4
    batches = [_ids(B, Ts, 70 + k) for k in range(6)]
    args = (S, REF_DB, MAX_DB, POWER, n_iter, win, hop)

    def run(serial):
        eng = pkg().Engine(hparams)
        try:
            eng.load_weights(weights)
            dev = [eng.to_device(ids) for ids in batches]
            outs = []
            for k, d in enumerate(dev):
                if k == 3:
                    eng.set_option('gl_momentum', 990)
                outs.append(eng.synthesize(d, *args, seed=90 + k, peak_normalize=True)['wav'])
                if serial:
                    eng.synchronize()
            eng.synchronize()
            return [o.to_host() for o in outs]
        finally:
            eng.close()

    back_to_back, waited = run(False), run(True)
    for k in range(len(batches)):
        assert np.isfinite(waited[k]).all() and np.abs(waited[k]).max() > 0
        assert np.array_equal(_bits(back_to_back[k]), _bits(waited[k])), k


@pytest.mark.parametrize('win,hop,n_fft', [(1102, 275, 2048), (800, 200, 1024)], ids=['streaming', 'general'])
def test_momentum_nan_stays_in_its_utterance(engine, win, hop, n_fft):
    """one NaN magnitude in utterance 1 of 2: that waveform is non-finite and its mse NaN (the NaN goes through the
    previous projection like through the phasor), utterance 0 keeps the bits of the clean run"""
    rng = np.random.default_rng(win + n_fft)
    B, F, T = 2, 1 + n_fft // 2, 40
    mag = C.power4_mag(rng, (B, F, T))
    init = rng.random((B, F, T)).astype(np.float32)
    wav0, mse0 = _gl(engine, mag, 4, win, hop, n_fft, init=init, gl_momentum=990)
    assert np.isfinite(wav0).all() and np.isfinite(mse0).all()
    dirty = mag.copy()
    dirty[1, F // 3, T // 2] = np.nan
    wav1, mse1 = _gl(engine, dirty, 4, win, hop, n_fft, init=init, gl_momentum=990)
    assert not np.isfinite(wav1[1]).all() and np.isnan(mse1[1])
    assert np.array_equal(_bits(wav1[0]), _bits(wav0[0])) and _bits(mse1)[0] == _bits(mse0)[0]


@pytest.mark.parametrize('stage', ['gl_stream', 'gl_general_1024'])
def test_momentum_beside_gemm_launches_of_another_handle(engine, neighbour, stage):  # noqa: F811
    """the momentum forms of the streaming and the general kernel under the neighbour of test_gpu_neighbours.py, with its
    repetition count: the bits of the quiet run"""
    eng2, launch = neighbour
    n_fft, win, hop, T, n_iter = {'gl_general_1024': (1024, 800, 200, 100, 3), 'gl_stream': (2048, 1102, 275, 200, 3)}[stage]
    rng = np.random.default_rng(11)
    mag = engine.to_device((rng.random((16, 1 + n_fft // 2, T), dtype=np.float32) ** 4) * 10)
    run = lambda: engine.griffin_lim(mag, n_iter, win, hop, n_fft, seed=3, want_mse=False)[0]   # noqa: E731
    try:
        engine.set_option('gl_momentum', 990)
        quiet = run()
        engine.synchronize()
        ref = quiet.to_host().copy()
        assert np.isfinite(ref).all()
        bad = n = 0
        for _ in range(25):
            launch()
            outs = [run() for _ in range(2)]
            engine.synchronize()
            eng2.synchronize()
            for o in outs:
                n += 1
                bad += not np.array_equal(o.to_host(), ref)
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
    finally:
        engine.set_option('gl_momentum', 0)
        mag.free()


def test_momentum_halves_the_iterations_on_the_shipped_spectrogram(engine):
    """What the option is for (frames 100:400 of the reference's own spectrogram, explicit phases): the mse after 30
    iterations at alpha = 0.99 is below the mse after 60 plain ones, on the GPU as in test_momentum_host.py"""
    mag, init = M.shipped_spectrogram()
    _, fast = _gl(engine, mag[None], 30, init=init[None], gl_momentum=990)
    _, plain = _gl(engine, mag[None], 60, init=init[None])
    print('mse: alpha 0.99 after 30 iterations {}, alpha 0 after 60 {}'.format(fast[0], plain[0]))
    assert np.isfinite(fast[0]) and fast[0] < plain[0]
