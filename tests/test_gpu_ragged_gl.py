"""GPU: tts_griffin_lim_ragged -- utterances of different lengths in one padded batch (reference audio/synthesis.py:43-125 per
utterance; datasets/statistics.py:146-187 for the reconstruction error).

The contract: utterance b's samples are the BITS of the single-utterance call tts_griffin_lim(B = 1, T = n_frames[b]) on its
own columns with the same handle options, whatever else is in the batch and whatever the padding columns hold; the rest of
its row is 0; its mse agrees with that call's (bit for bit where the partial sums are per frame: momentum, general kernels).
The shapes are the smallest at which this can go wrong: 5 frames is the shortest legal utterance at 1102 / 275, 8 and 9
straddle "no interior frame" (2 halo + 1 = 9), a long utterance is followed by a short one.  Inputs and float64 references:
ragged_cases.py (test_ragged_gl_host.py holds a float32 restatement to a quarter of the bounds on the same inputs)."""
import os

import numpy as np
import pytest

import audio_cases as C
import ragged_cases as R
from conftest import pkg, rel_l2
from oracle import audio_oracle as A
from parity import assert_segment_parity
from test_gpu_audio import seed_u

pytestmark = pytest.mark.gpu

_SINGLE = {}


def single(engine, cfg, T, n_iter, want_mse, per_launch=3, momentum=None, init=None, key=None):
    """the single-utterance call (B = 1, T = the utterance's frames) on the utterance's own arrays; once per form"""
    k = (cfg, T, n_iter, want_mse, per_launch, momentum, key)
    if k not in _SINGLE:
        n_fft, win, hop = cfg
        mag, own = R.utterance(cfg, T)
        u = own if init is None else init
        engine.set_option('gl_pair', per_launch)
        try:
            wav, mse = engine.griffin_lim(mag[None], n_iter, win, hop, n_fft, init_phase=u[None], want_mse=want_mse, momentum=momentum)
        finally:
            engine.set_option('gl_pair', 3)
        _SINGLE[k] = (wav.to_host()[0], mse.to_host()[0] if want_mse else None)
    return _SINGLE[k]


def ragged(engine, cfg, mag, init, lengths, n_iter, want_mse, per_launch=3, momentum=None, seed=0):
    n_fft, win, hop = cfg
    engine.set_option('gl_pair', per_launch)
    try:
        wav, mse = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=init, seed=seed, want_mse=want_mse, momentum=momentum,
                                      n_frames=lengths)
    finally:
        engine.set_option('gl_pair', 3)
    return wav.to_host(), (mse.to_host() if want_mse else None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_against_singles(engine, cfg, lengths, wav, mse, n_iter, want_mse, per_launch=3, momentum=None, mse_bits=False, label=''):
    hop = cfg[2]
    assert wav.shape == (len(lengths), hop * (max(lengths) - 1))
    for b, T in enumerate(lengths):
        n = hop * (T - 1)
        one_wav, one_mse = single(engine, cfg, T, n_iter, want_mse, per_launch, momentum)
        assert np.array_equal(bits(wav[b, :n]), bits(one_wav)), '{} b={} T={}: not the bits of the single-utterance call'.format(label, b, T)
        assert not wav[b, n:].any() and not np.signbit(wav[b, n:]).any(), '{} b={}: the row tail is not 0.0'.format(label, b)
        if want_mse:
            print('{} b={} T={}: mse {!r} single {!r}'.format(label, b, T, mse[b], one_mse))
            if mse_bits:
                assert bits(mse[b]) == bits(one_mse)
            else:
                assert abs(mse[b] - one_mse) <= 1e-3 * abs(one_mse) + 1e-9


def check_against_oracle(cfg, lengths, wav, mse, n_iter, want_mse, momentum=0.0, label=''):
    hop = cfg[2]
    for b, T in enumerate(lengths):
        ref_wav, ref_mse = R.reference(cfg, T, n_iter, momentum=momentum)
        assert_segment_parity(wav[b, :hop * (T - 1)], ref_wav, hop, C.gl_tol(n_iter), '{} b={} T={}'.format(label, b, T))
        if want_mse and n_iter > 0:
            assert abs(mse[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9


# ---------------------------------------------------------------------------------------------- streaming kernel
@pytest.mark.parametrize('per_launch', [1, 2, 3])
@pytest.mark.parametrize('n_iter,want_mse', [(0, False), (1, False), (4, True), (7, False)])
def test_streaming_ragged_is_the_single_utterance_call_bit_for_bit(engine, n_iter, want_mse, per_launch):
    lengths = R.STREAM_LENGTHS
    mag, init = R.batch(R.STREAM, lengths)
    label = 'ragged 1102/275 it={} pair={}'.format(n_iter, per_launch)
    wav, mse = ragged(engine, R.STREAM, mag, init, lengths, n_iter, want_mse, per_launch)
    check_against_singles(engine, R.STREAM, lengths, wav, mse, n_iter, want_mse, per_launch, label=label)
    check_against_oracle(R.STREAM, lengths, wav, mse, n_iter, want_mse, label=label)


@pytest.mark.parametrize('per_launch', [1, 2, 3])
@pytest.mark.parametrize('n_iter,want_mse', [(0, False), (4, True), (7, False)])
def test_padding_never_reaches_a_result(engine, n_iter, want_mse, per_launch):
    """every padding column of mag and init_phase set to NaN: the outputs are the bits of the clean call"""
    lengths = R.STREAM_LENGTHS
    mag, init = R.batch(R.STREAM, lengths)
    clean_wav, clean_mse = ragged(engine, R.STREAM, mag, init, lengths, n_iter, want_mse, per_launch)
    mag_n, init_n = R.batch(R.STREAM, lengths, fill=np.nan)
    assert np.isnan(mag_n).sum() == sum(1025 * (max(lengths) - T) for T in lengths)
    wav, mse = ragged(engine, R.STREAM, mag_n, init_n, lengths, n_iter, want_mse, per_launch)
    assert np.isfinite(wav).all()
    assert np.array_equal(bits(wav), bits(clean_wav))
    if want_mse:
        assert np.array_equal(bits(mse), bits(clean_mse))


def test_a_nan_inside_an_utterance_stays_in_that_utterance(engine):
    lengths = R.STREAM_LENGTHS
    mag, init = R.batch(R.STREAM, lengths)
    clean_wav, clean_mse = ragged(engine, R.STREAM, mag, init, lengths, 4, True)
    mag[1, 300, 3] = np.nan
    wav, mse = ragged(engine, R.STREAM, mag, init, lengths, 4, True)
    n1 = 275 * (lengths[1] - 1)
    assert not np.isfinite(wav[1, :n1]).all() and not np.isfinite(mse[1])
    assert not wav[1, n1:].any()
    for b in (0, 2, 3, 4):
        assert np.array_equal(bits(wav[b]), bits(clean_wav[b])) and bits(mse[b]) == bits(clean_mse[b])


@pytest.mark.parametrize('n_iter,want_mse,per_launch', [(4, True, 3), (7, False, 2), (1, False, 1)])
def test_forced_cuts_do_not_reach_the_bits(engine, n_iter, want_mse, per_launch):
    """runs of 8 frames on 16 workgroups: the 40-frame utterance in five runs, the 23-frame one in three"""
    lengths = R.STREAM_LENGTHS
    mag, init = R.batch(R.STREAM, lengths)
    engine.set_option('debug_hooks', 1)
    try:
        engine.set_option('gl_run_len', 8)
        engine.set_option('gl_workers', 16)
        wav, mse = ragged(engine, R.STREAM, mag, init, lengths, n_iter, want_mse, per_launch)
    finally:
        for k in ('gl_run_len', 'gl_workers', 'debug_hooks'):
            engine.set_option(k, 0)
    check_against_singles(engine, R.STREAM, lengths, wav, mse, n_iter, want_mse, per_launch, label='forced cut it={}'.format(n_iter))


@pytest.mark.parametrize('n_iter,want_mse,per_launch', [(0, False, 3), (1, False, 1), (4, True, 3), (7, False, 3)])
def test_seeded_start_draws_as_the_padded_layout_does(engine, n_iter, want_mse, per_launch):
    """init_phase == NULL: bin (b, f, t) is drawn as tts_griffin_lim(B, T_max, seed) draws it.  Compared with the explicit-phase
    ragged call fed the numpy restatement of those draws, at the bound test_gpu_audio.py::test_griffin_lim_seeded_start
    uses for the same pair (the v_sin / v_cos error of the in-kernel draw), and with the oracle per utterance."""
    seed = 7
    lengths = R.STREAM_LENGTHS
    mag, _ = R.batch(R.STREAM, lengths)
    u = seed_u(seed, len(lengths), 1025, max(lengths))
    w_seed, m_seed = ragged(engine, R.STREAM, mag, None, lengths, n_iter, want_mse, per_launch, seed=seed)
    w_expl, m_expl = ragged(engine, R.STREAM, mag, u, lengths, n_iter, want_mse, per_launch)
    w_again, _ = ragged(engine, R.STREAM, mag, None, lengths, n_iter, want_mse, per_launch, seed=seed)
    assert np.array_equal(bits(w_seed), bits(w_again))
    tol = 4e-5 * max(1, n_iter)
    for b, T in enumerate(lengths):
        n = 275 * (T - 1)
        assert not w_seed[b, n:].any()
        assert rel_l2(w_seed[b, :n], w_expl[b, :n]) < tol, (b, rel_l2(w_seed[b, :n], w_expl[b, :n]))
        ref_wav, ref_mse = R.reference(R.STREAM, T, n_iter, init=u[b, :, :T], key=('seed', seed, b, max(lengths)))
        assert rel_l2(w_seed[b, :n], ref_wav) < 1e-4 * max(1, n_iter)
        if want_mse:
            assert abs(m_seed[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9


@pytest.mark.parametrize('cfg,T,n_iter', [(R.STREAM, 23, 4), (R.STREAM, 9, 7), (R.STREAM_800, 30, 4), (R.GENERAL_1024, 25, 3)])
@pytest.mark.parametrize('seeded', [False, True])
def test_uniform_lengths_through_the_ragged_entry_are_tts_griffin_lim(engine, cfg, T, n_iter, seeded):
    n_fft, win, hop = cfg
    B = 3
    rng = np.random.default_rng(T)
    mag = C.power4_mag(rng, (B, 1 + n_fft // 2, T))
    init = None if seeded else rng.random(mag.shape).astype(np.float32)
    want_mse = n_iter == 4 or n_iter == 3
    ref_wav, ref_mse = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=init, seed=5, want_mse=want_mse)
    wav, mse = ragged(engine, cfg, mag, init, [T] * B, n_iter, want_mse, seed=5)
    assert np.array_equal(bits(wav), bits(ref_wav.to_host()))
    if want_mse:
        assert np.array_equal(bits(mse), bits(ref_mse.to_host()))


@pytest.mark.parametrize('per_launch', [1, 3])
def test_second_window_ragged(engine, per_launch):
    lengths = R.STREAM_800_LENGTHS
    mag, init = R.batch(R.STREAM_800, lengths, fill=np.nan)
    wav, mse = ragged(engine, R.STREAM_800, mag, init, lengths, 4, True, per_launch)
    check_against_singles(engine, R.STREAM_800, lengths, wav, mse, 4, True, per_launch, label='ragged 800/200 pair={}'.format(per_launch))
    check_against_oracle(R.STREAM_800, lengths, wav, mse, 4, True, label='ragged 800/200')


# ---------------------------------------------------------------------------------------------- general kernels
@pytest.mark.parametrize('cfg,lengths', [(R.GENERAL_1024, R.GENERAL_1024_LENGTHS), (R.GENERAL_512, R.GENERAL_512_LENGTHS)],
                         ids=['1024', '512'])
@pytest.mark.parametrize('n_iter,want_mse', [(0, False), (3, True)])
def test_general_kernels_ragged(engine, cfg, lengths, n_iter, want_mse):
    """one workgroup per frame: the workgroups of padding frames leave, the gather and the reflect padding stop at the
    utterance's end; the mse partials are per frame, so the mse is the single call's bit for bit.  Padding = NaN."""
    mag, init = R.batch(cfg, lengths, fill=np.nan)
    label = 'ragged general {} it={}'.format(cfg, n_iter)
    wav, mse = ragged(engine, cfg, mag, init, lengths, n_iter, want_mse)
    check_against_singles(engine, cfg, lengths, wav, mse, n_iter, want_mse, mse_bits=True, label=label)
    check_against_oracle(cfg, lengths, wav, mse, n_iter, want_mse, label=label)


# ---------------------------------------------------------------------------------------------- momentum
@pytest.mark.parametrize('cfg,lengths', [(R.STREAM, R.MOMENTUM_LENGTHS), (R.GENERAL_1024, R.GENERAL_1024_LENGTHS)], ids=['stream', '1024'])
def test_momentum_ragged(engine, cfg, lengths):
    """alpha = 0.99, four iterations: the squared error is kept per frame, so waveform AND mse are the bits of the
    single-utterance momentum calls; parity with tests/momentum_oracle.py at the bound test_gpu_momentum.py uses"""
    n_iter = 4
    mag, init = R.batch(cfg, lengths, fill=np.nan)
    wav, mse = ragged(engine, cfg, mag, init, lengths, n_iter, True, momentum=R.MOMENTUM)
    check_against_singles(engine, cfg, lengths, wav, mse, n_iter, True, momentum=R.MOMENTUM, mse_bits=True, label='ragged momentum {}'.format(cfg))
    check_against_oracle(cfg, lengths, wav, mse, n_iter, True, momentum=R.MOMENTUM, label='ragged momentum {}'.format(cfg))


def test_refusals_name_the_utterance(engine):
    """through the C entry point itself (the Python wrapper checks the same things first): nothing is enqueued"""
    import ctypes
    H = pkg('_hip')
    mag = engine.to_device(np.ones((3, 1025, 12), np.float32))
    wav = engine.empty((3, 275 * 11))
    try:
        for bad, word in [([12, 0, 9], 'n_frames[1]'), ([12, 9, 13], 'n_frames[2]'), ([4, 9, 12], 'utterance 0')]:
            nf = np.array(bad, np.int32)
            rc = engine.lib.tts_griffin_lim_ragged(engine.handle, mag.data_ptr(), None, 0, 3, 12, nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                   2, 1102, 275, 2048, wav.data_ptr(), None)
            assert rc == H.TTS_ERR_INVALID
            with pytest.raises(H.TtsError, match=word.replace('[', r'\[').replace(']', r'\]')):
                engine._check(rc)
        with pytest.raises(ValueError):
            engine.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=[12, 9])
        with pytest.raises(ValueError):
            engine.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=[12, 9, 9], momentum=1.0)
    finally:
        mag.free()
        wav.free()


# ---------------------------------------------------------------------------------------------- beside other work
def test_ragged_call_beside_gemm_launches_of_another_handle(engine, hparams, weights):
    """as tests/test_gpu_neighbours.py runs every other stage: MFMA GEMM waves of a second handle on the chip, the same bits
    over its repetitions"""
    eng2 = pkg().Engine(hparams)
    eng2.load_weights(weights)
    rng = np.random.default_rng(7)
    x = eng2.to_device(rng.standard_normal((9600, 256)).astype(np.float32))
    w = eng2.to_device(rng.standard_normal((256, 256)).astype(np.float32))
    c = eng2.empty((9600, 256))
    lengths = [int(round(v)) for v in np.linspace(60, 200, 16)]
    mag_h = np.zeros((16, 1025, 200), np.float32)
    for b, T in enumerate(lengths):
        mag_h[b, :, :T] = C.power4_mag(np.random.default_rng(11 + b), (1025, T))
    mag = engine.to_device(mag_h)
    run = lambda: engine.griffin_lim(mag, 3, 1102, 275, 2048, seed=3, want_mse=False, n_frames=lengths)[0]   # noqa: E731
    try:
        quiet = run()
        engine.synchronize()
        ref = quiet.to_host().copy()
        assert np.isfinite(ref).all() and ref[0, :275 * 59].any() and not ref[0, 275 * 59:].any()
        bad = n = 0
        for _ in range(25):
            for _ in range(30):
                eng2._check(eng2.lib.tts_debug_gemm(eng2.handle, x.data_ptr(), w.data_ptr(), c.data_ptr(), 9600, 256, 256, 1, 150, 0))
            outs = [run() for _ in range(2)]
            engine.synchronize()
            eng2.synchronize()
            for o in outs:
                n += 1
                bad += not np.array_equal(o.to_host(), ref)
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
    finally:
        eng2.synchronize()
        for a in (x, w, c):
            a.free()
        mag.free()
        eng2.close()


# ---------------------------------------------------------------------------------------------- statistics, GTA waveforms
def test_collect_reconstruction_error_is_the_mean_of_the_oracles(engine, tmp_path):
    ST = pkg('datasets.statistics')
    io = pkg('audio.io')
    n_iters, sr = 3, 22050
    rng = np.random.default_rng(5)
    paths, init, expect = [], {}, []
    for k, n in enumerate([3300, 1400, 5100]):
        wav = C.tone_noise(rng, n, k)
        p = str(tmp_path / 'r{}.wav'.format(k))
        io.save_wav(p, wav, sr)
        loaded, rate = io.load_wav(p)
        assert rate == sr and len(loaded) == n
        mag = np.abs(A.stft(np.asarray(loaded, np.float32), 2048, 275, 1102)).astype(np.float32)
        init[p] = rng.random(mag.shape).astype(np.float32)
        expect.append(A.griffin_lim_v2(mag, 1102, 275, 2048, n_iters, init_phase=init[p])[1])
        paths.append(p)
    total = ST.collect_reconstruction_error(paths, n_iters, batch_size=32, engine=engine, init_phases=init)
    print('reconstruction error {} vs oracle mean {}'.format(total, np.mean(expect)))
    assert abs(total - np.mean(expect)) <= 1e-3 * abs(np.mean(expect))


def test_gta_wav_writes_files_of_the_utterances_own_lengths(engine, hparams, tmp_path, monkeypatch):
    """tacotron.gta with_wav on a small corpus: one .gta.wav beside every .gta.npz, hop (T_red r - 1) samples each"""
    G = pkg('tacotron.gta')
    P = pkg('tacotron.params')
    M = pkg('tacotron.model')
    io = pkg('audio.io')
    monkeypatch.setattr(P.evaluation_params, 'n_buckets', 2)
    r, nm, F = hparams.reduction, hparams.n_mels, 1 + hparams.n_fft // 2
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'wavs'))
    rows = [('LJ00{}'.format(i), text) for i, text in enumerate(['a cat', 'hi there', 'a longer sentence', 'dogs', 'the end'])]
    rng = np.random.default_rng(0)
    t_red = {}
    with open(os.path.join(root, 'metadata.csv'), 'w') as f:
        for i, (fid, text) in enumerate(rows):
            f.write('{}|{}|{}\n'.format(fid, text.upper(), text))
            t_red[fid] = 2 + i % 4
            np.savez(os.path.join(root, 'wavs', fid + '.npz'), mel_mag_db=rng.random((t_red[fid], nm * r)).astype(np.float32),
                     linear_mag_db=rng.random((t_red[fid], F * r)).astype(np.float32))
    dataset = pkg('datasets.lj_speech').LJSpeechDatasetHelper(root, P.dataset_params.vocabulary_dict, False)
    model = M.Tacotron(M.Tacotron.model_placeholders(), M.Mode.PREDICT, hparams=hparams, engine=engine)
    out_dir = str(tmp_path / 'gta')
    res = G.write_gta(model, G.batches_with_paths(dataset, None, 3, verbose=False), out_dir, verbose=False, with_wav=True, gl_iters=2)
    assert res['n_files'] == len(rows)
    hop = int(hparams.win_hop / 1000 * hparams.sampling_rate)
    assert sorted(os.listdir(out_dir)) == sorted([fid + '.gta.npz' for fid, _ in rows] + [fid + '.gta.wav' for fid, _ in rows])
    for fid, _ in rows:
        wav, sr = io.load_wav(os.path.join(out_dir, fid + '.gta.wav'))
        assert sr == hparams.sampling_rate and len(wav) == hop * (t_red[fid] * r - 1), (fid, len(wav))
        assert np.isfinite(wav).all() and abs(np.abs(wav).max() - 1.0) < 1e-6   # peak-normalised
