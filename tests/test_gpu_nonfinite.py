"""GPU: a NaN that enters the audio surface comes out as a NaN -- never as a quiet, plausible bin -- and touches nothing
that does not depend on it (the rule of include/sstts_hip.h, "Non-finite values on the audio side").

The reference's np.clip / np.maximum / np.power path (tacotron/inference.py:93-101, audio/conversion.py) carries a NaN into
the waveform; fminf / fmaxf return their OTHER operand for a NaN, so a clip written with them turns the NaN of a corrupt
checkpoint or of an overflow upstream into the -93.87 dB floor and the library returns a finite waveform.  +-Inf clip like
any other value, as in numpy.
"""
import numpy as np
import pytest

from conftest import pkg
from oracle import audio_oracle as A

pytestmark = pytest.mark.gpu
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3
NAN = np.float32(np.nan)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_denorm_power_carries_nan_and_clips_infinities(engine):
    rng = np.random.default_rng(50)
    B, T, F = 3, 31, 1025
    lin = (rng.random((B, T, F)) * 1.4 - 0.2).astype(np.float32)
    clean = engine.denorm_power(lin, REF_DB, MAX_DB, POWER).to_host()
    dirty_in = lin.copy()
    dirty_in[1, 7, 300] = NAN
    dirty_in[2, 30, 1024] = np.inf
    dirty_in[0, 0, 0] = -np.inf
    dirty = engine.denorm_power(dirty_in, REF_DB, MAX_DB, POWER).to_host()
    assert np.isnan(dirty[1, 300, 7])                                   # (B, F, T): the transposed position
    with np.errstate(invalid='ignore'):
        ref = np.stack([A.linear_to_magnitude(dirty_in[b], REF_DB, MAX_DB, POWER) for b in range(B)])
    assert np.isnan(ref[1, 300, 7]) and np.isnan(ref).sum() == 1       # what numpy does
    assert np.isnan(dirty).sum() == 1
    assert abs(dirty[2, 1024, 30] / ref[2, 1024, 30] - 1) <= 2e-5      # +Inf clips to 1
    assert abs(dirty[0, 0, 0] / ref[0, 0, 0] - 1) <= 2e-5              # -Inf clips to 0
    touched = np.zeros(clean.shape, bool)
    touched[1, 300, 7] = touched[2, 1024, 30] = touched[0, 0, 0] = True
    assert np.array_equal(_bits(dirty)[~touched], _bits(clean)[~touched])


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_db_convert_carries_nan(engine, mode):
    """np.maximum(1e-5, nan), np.power(10, nan / 20) and np.clip(nan, 0, 1) are NaN: NaN in, NaN out, in every mode; the
    neighbours keep the bits of a clean run; a NaN does not trip mode 1's range check"""
    rng = np.random.default_rng(mode)
    n = 4096 * 256 + 1
    x = {0: rng.random(n) * 3, 1: rng.random(n) * 100 - 90, 2: rng.random(n) * 200 - 150, 3: rng.random(n) * 1.4 - 0.2}[mode]
    x = x.astype(np.float32)
    clean = engine.db_convert(x, mode, REF_DB, MAX_DB)
    at = [0, 255, 256, n // 2, n - 1]
    xd = x.copy()
    xd[at] = NAN
    xd[1] = -NAN                                                        # either sign bit
    dirty = engine.db_convert(xd, mode, REF_DB, MAX_DB)
    assert np.isnan(dirty[at]).all() and np.isnan(dirty[1]) and np.isnan(dirty).sum() == len(at) + 1
    keep = np.ones(n, bool)
    keep[at + [1]] = False
    assert np.array_equal(_bits(dirty)[keep], _bits(clean)[keep])


def test_peak_normalize_keeps_nan_in_its_row(engine):
    rng = np.random.default_rng(51)
    wav = (rng.standard_normal((4, 5000)) * 0.01).astype(np.float32)
    clean = engine.peak_normalize(engine.to_device(wav)).to_host()
    dirty_in = wav.copy()
    dirty_in[2, 1234] = NAN
    dirty = engine.peak_normalize(engine.to_device(dirty_in)).to_host()
    assert np.isnan(dirty[2]).any() and np.isnan(dirty[2, 1234])
    for b in (0, 1, 3):
        assert np.array_equal(_bits(dirty[b]), _bits(clean[b])), b


@pytest.mark.parametrize('win,hop,n_fft,T', [(1102, 275, 2048, 40), (800, 200, 2048, 40), (800, 200, 1024, 40)])
def test_griffin_lim_nan_stays_in_its_utterance(engine, win, hop, n_fft, T):
    """One NaN magnitude in utterance 1 of 3 (the streaming kernel's two instantiations and the general kernels): its
    waveform is non-finite and its mse NaN; utterances 0 and 2 keep the bits of the clean run.  No loop bound and no wait
    of these kernels depends on the data -- the streaming kernel waits on its frame-index chain and its work counter, the
    general kernels loop over indices only -- so a NaN cannot stall them."""
    rng = np.random.default_rng(win + n_fft)
    B, F = 3, 1 + n_fft // 2
    mag = ((rng.random((B, F, T)) ** 4) * 10).astype(np.float32)
    init = rng.random((B, F, T)).astype(np.float32)
    wav0, mse0 = engine.griffin_lim(mag, 3, win, hop, n_fft, init_phase=init, want_mse=True)
    wav0, mse0 = wav0.to_host(), mse0.to_host()
    assert np.isfinite(wav0).all() and np.isfinite(mse0).all()
    dirty = mag.copy()
    dirty[1, F // 3, T // 2] = NAN
    wav1, mse1 = engine.griffin_lim(dirty, 3, win, hop, n_fft, init_phase=init, want_mse=True)
    wav1, mse1 = wav1.to_host(), mse1.to_host()
    assert not np.isfinite(wav1[1]).all()
    assert np.isnan(mse1[1])
    for b in (0, 2):
        assert np.array_equal(_bits(wav1[b]), _bits(wav0[b])), b
        assert _bits(mse1[b:b + 1])[0] == _bits(mse0[b:b + 1])[0], b


def test_fused_epilogue_carries_a_nan_bias_like_the_staged_path(hparams, weights):
    """tts_synthesize de-normalises in the final Dense's GEMM epilogue (csrc/gemm_f32.hip), tts_postnet_forward +
    tts_denorm_power in a kernel of its own: with one NaN entry in the final Dense's bias both give NaN in that bin of
    every frame and the same finite magnitudes elsewhere."""
    w = dict(weights)
    bias = w['dense/bias'].copy()
    k = 417
    bias[k] = NAN
    w['dense/bias'] = bias
    eng = pkg().Engine(hparams)
    try:
        eng.load_weights(w)
        rng = np.random.default_rng(52)
        B, Ts, S = 2, 13, 4
        T, F, FP = S * hparams.reduction, 1025, 1056
        ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
        ids[:, -1] = 1
        eng.set_option('pipeline', 0)
        out = eng.synthesize(ids, S, REF_DB, MAX_DB, POWER, 1, 1102, 275, seed=3, peak_normalize=False, want_mel=True,
                             want_linear=True)
        eng.synchronize()
        fused = eng.debug_workspace('gl.mag', (B, T, FP))[:, :, :F]           # frame-major, rows padded to FP
        lin_fused = out['linear'].to_host()
        mel = out['mel'].to_host()
        wav = out['wav'].to_host()
        lin = eng.postnet_forward(mel.reshape(B, T, hparams.n_mels)).to_host()
        staged = eng.denorm_power(lin, REF_DB, MAX_DB, POWER).to_host().transpose(0, 2, 1)   # (B, F, T) -> (B, T, F)
    finally:
        eng.close()
    expect = np.zeros((B, T, F), bool)
    expect[:, :, k] = True
    assert np.array_equal(np.isnan(lin), expect) and np.array_equal(np.isnan(lin_fused), expect)
    assert np.array_equal(np.isnan(staged), expect), 'staged: NaN bins {}'.format(int(np.isnan(staged).sum()))
    assert np.array_equal(np.isnan(fused), expect), 'fused: NaN bins {}'.format(int(np.isnan(fused).sum()))
    assert np.isfinite(fused[~expect]).all() and np.isfinite(staged[~expect]).all()
    assert np.allclose(fused[~expect], staged[~expect], rtol=2e-5, atol=0)
    assert not np.isfinite(wav).all()                                        # and the waveform says so
