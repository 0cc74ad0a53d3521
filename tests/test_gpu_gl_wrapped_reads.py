"""GPU: the wrapped linear read of the streaming Griffin-Lim kernel's forward-transform input (griffin_lim.hip, fft_input).

An interior frame whose span crosses the end of the ring after the next lap's fold (ring slots R - 4 ... R - 1 at 1102 / 275)
reads its slots at or above the end of the ring ring_len lower and the straddling slot element by element; every other
interior frame reads linearly as before.  Which ring slot a frame sits on depends on where its run starts, so between two
cuts of an utterance into runs a given frame is read by the one path in one cut and by the other in the other: equal
waveform BITS across cuts hold the two paths to each other, the oracle holds the uncut call.  Shapes: the smallest that
reach ring slots R - 4 ... R - 1 and the lap after them at every number of iterations per launch (R = 24 / 38 / 64 at
1102 / 275, tests/test_gl_wrapped_reads.py has the arithmetic)."""
import numpy as np
import pytest

import audio_cases as C
from oracle import audio_oracle as A
from test_gpu_audio import gl_segments   # the per-sample, per-segment bound test_gpu_audio.py holds this comparison to

pytestmark = pytest.mark.gpu

N_FFT, B, N_ITER = 2048, 2, 6   # six iterations: every stage form (3 + 3, 2 + 2 + 2, six of one) runs at least twice


def _cuts(engine, mag, init, win, hop, per_launch, cuts, **kw):
    """-> {cut: waveform} of one call per cut; cut = (gl_runs, gl_run_len)"""
    d_mag, d_init = engine.to_device(mag), engine.to_device(init)
    outs = {}
    engine.set_option('gl_pair', per_launch)
    engine.set_option('debug_hooks', 1)
    try:
        for runs, run_len in cuts:
            engine.set_option('gl_runs', runs)
            engine.set_option('gl_run_len', run_len)
            wav, _ = engine.griffin_lim(d_mag, N_ITER, win, hop, N_FFT, init_phase=d_init, want_mse=False, **kw)
            engine.synchronize()
            outs[(runs, run_len)] = wav.to_host().copy()
            wav.free()
    finally:
        for k in ('gl_runs', 'gl_run_len', 'debug_hooks'):
            engine.set_option(k, 0)
        engine.set_option('gl_pair', 3)
        d_mag.free(); d_init.free()
    return outs


def _same_bits(outs, label):
    ref = outs[(1, 0)]
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    for k, v in outs.items():
        assert np.array_equal(ref.view(np.uint32), v.view(np.uint32)), (label, k)
    return ref


@pytest.mark.parametrize('win,hop,T,per_launch,run_lens', [
    (1102, 275, 75, 3, (8, 24, 40)),    # R = 24
    (1102, 275, 100, 2, (8, 24, 40)),   # R = 38
    (1102, 275, 160, 1, (8, 24, 40)),   # R = 64
    (800, 200, 130, 3, (8, 24, 40)),    # R = 34
])
def test_cut_does_not_reach_the_bits_and_the_uncut_call_matches_the_oracle(engine, win, hop, T, per_launch, run_lens):
    rng = np.random.default_rng(1000 * per_launch + T)
    mag = C.synth_mag(rng, B, T, hop=hop, win=win)
    init = rng.random(mag.shape).astype(np.float32)
    outs = _cuts(engine, mag, init, win, hop, per_launch, [(1, 0)] + [(0, n) for n in run_lens])
    wav = _same_bits(outs, (win, hop, T, per_launch))
    for b in range(B):
        ref_wav, _ = A.griffin_lim_v2(mag[b], win, hop, N_FFT, N_ITER, init_phase=init[b])
        assert wav[b].shape == ref_wav.shape
        gl_segments(wav[b], ref_wav, hop, N_ITER, 'GL wrapped reads {}/{} T={} {} per launch b={}'.format(win, hop, T, per_launch, b))


def test_ragged_call_same_bits_across_cuts(engine):
    """tts_griffin_lim_ragged, lengths 75 and 52 (the RAG instantiations, three iterations per launch)"""
    T, lens = 75, [75, 52]
    rng = np.random.default_rng(7552)
    mag = C.synth_mag(rng, B, T)
    init = rng.random(mag.shape).astype(np.float32)
    outs = _cuts(engine, mag, init, 1102, 275, 3, [(1, 0), (0, 24)], n_frames=lens)
    wav = _same_bits(outs, 'ragged')
    for b in range(B):
        assert np.abs(wav[b, :275 * (lens[b] - 1)]).max() > 0 and not wav[b, 275 * (lens[b] - 1):].any()


def test_momentum_call_same_bits_across_cuts(engine):
    """fast Griffin-Lim (gl_momentum: the MOM instantiations, one iteration per launch, R = 64)"""
    T = 160
    rng = np.random.default_rng(160)
    mag = C.synth_mag(rng, B, T)
    init = rng.random(mag.shape).astype(np.float32)
    outs = _cuts(engine, mag, init, 1102, 275, 1, [(1, 0), (0, 40)], momentum=0.99)
    _same_bits(outs, 'momentum')
