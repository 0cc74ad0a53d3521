"""CPU: the bounds the GPU audio tests hold per bin, frame, channel and hop segment are FAIR on the inputs those tests use.

A float32 restatement of every operation (audio_cases.stft32 / magnitude32 / mel32 / griffin_lim32: torch on the CPU) is
compared with the float64 oracle over the tables of audio_cases.py -- the very signals, magnitudes and initial phases of
test_gpu_analysis.py and of the Griffin-Lim tests of test_gpu_audio.py / test_gpu_edge_cases.py -- and every per-slice
figure has to stay within a QUARTER of the bound the GPU test uses (1e-5 on the analysis side; 1e-4 max(1, n_iter) for
a Griffin-Lim waveform).  Plain float32 arithmetic therefore has a fourfold margin: a kernel that misses the bound is
wrong, not unlucky, and an input on which float32 itself came near the bound would show up here.
"""
import numpy as np
import pytest

import audio_cases as C
from oracle import audio_oracle as A
from parity import assert_parity, assert_segment_parity

QUARTER = C.HOST_MARGIN


@pytest.mark.parametrize('kind', sorted(C.SIGNALS))
@pytest.mark.parametrize('case', range(len(C.ANALYSIS_CASES)))
def test_float32_stft_magnitude_and_mel_within_a_quarter_of_the_bound(case, kind):
    n_fft, win, hop, n, B = C.ANALYSIS_CASES[case]
    y = C.signals(kind, case, B, n)
    ref = C.ref_stft(y, n_fft, win, hop)
    got = C.stft32(y, n_fft, win, hop)
    assert got.shape == ref.shape == (B, 1 + n_fft // 2, 1 + n // hop)
    label = 'f32 {} case {} {}'.format(kind, case, C.ANALYSIS_CASES[case])
    tol = QUARTER * C.ANALYSIS_TOL
    assert_parity(C.as_real(got), C.as_real(ref), C.STFT_AXES, tol, label + ' stft')
    for p in C.POWERS:
        assert_parity(C.magnitude32(got, p), np.abs(ref) ** p, C.STFT_AXES, tol, label + ' |S|^{}'.format(p))
    sr, _, n_mels, fmin, fmax = C.MEL_CONFIGS[0]
    lin = C.magnitude32(got, 1.0)
    rmel = np.matmul(A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax), np.abs(ref))
    assert_parity(C.mel32(lin, sr, n_fft, n_mels, fmin, fmax), rmel, C.MEL_AXES, tol, label + ' mel')


@pytest.mark.parametrize('B', C.MEL_BATCHES)
@pytest.mark.parametrize('n_frames', C.MEL_FRAMES)
@pytest.mark.parametrize('cfg', range(len(C.MEL_CONFIGS)))
def test_float32_mel_within_a_quarter_of_the_bound(cfg, n_frames, B):
    sr, n_fft, n_mels, fmin, fmax = C.MEL_CONFIGS[cfg]
    lin = C.mel_input(cfg, n_frames, B)
    ref = np.matmul(A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax), lin.astype(np.float64))
    assert_parity(C.mel32(lin, sr, n_fft, n_mels, fmin, fmax), ref, C.MEL_AXES, QUARTER * C.ANALYSIS_TOL,
                  'f32 mel cfg {} frames {} B {}'.format(cfg, n_frames, B))


def test_float32_filterbank_storage_is_within_the_identity_bound():
    """test_gpu_analysis.py reads the filter bank itself through lin = I and holds every entry to 1e-6 of the bank's
    maximum: float32 storage of the float64 bank is 6e-8 relative, a quarter of that bound with room"""
    for sr, n_fft, n_mels, fmin, fmax in C.MEL_CONFIGS:
        bank = A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        assert np.abs(bank.astype(np.float32).astype(np.float64) - bank).max() <= QUARTER * 1e-6 * bank.max()


def _gl_check(mag, init, win, hop, n_fft, n_iter, label):
    for b in range(mag.shape[0]):
        ref_wav, ref_mse = A.griffin_lim_v2(mag[b], win, hop, n_fft, n_iter, init_phase=init[b])
        wav, mse = C.griffin_lim32(mag[b], win, hop, n_fft, n_iter, init[b])
        tol = QUARTER * C.gl_tol(n_iter)
        assert np.linalg.norm(wav - ref_wav) / np.linalg.norm(ref_wav) < tol
        assert_segment_parity(wav, ref_wav, hop, tol, '{} b={}'.format(label, b))
        if n_iter > 0:
            assert abs(mse - ref_mse) <= QUARTER * 1e-3 * abs(ref_mse) + 1e-9


@pytest.mark.parametrize('B,T,n_iter', C.GL_FEW)
def test_float32_griffin_lim_few_iterations(B, T, n_iter):
    mag, init = C.gl_few_input(B, T, n_iter)
    _gl_check(mag, init, 1102, 275, 2048, n_iter, 'f32 GL few T={} it={}'.format(T, n_iter))


@pytest.mark.parametrize('B,T,n_iter,want_mse', C.GL_PER_LAUNCH)
def test_float32_griffin_lim_iterations_per_launch(B, T, n_iter, want_mse):
    mag, init = C.gl_per_launch_input(B, T, n_iter)
    _gl_check(mag, init, 1102, 275, 2048, n_iter, 'f32 GL per-launch T={} it={}'.format(T, n_iter))


@pytest.mark.parametrize('run_len', C.GL_RUN_LENS)
def test_float32_griffin_lim_forced_run_cuts(run_len):
    mag, init = C.gl_run_cut_input(run_len)
    for _, n_iter, _ in C.GL_RUN_CUT_FORMS:
        _gl_check(mag, init, 1102, 275, 2048, n_iter, 'f32 GL run cuts {} it={}'.format(run_len, n_iter))


@pytest.mark.parametrize('n_fft,win,hop,B,T', C.GL_OTHER_SIZES)
def test_float32_griffin_lim_other_sizes(n_fft, win, hop, B, T):
    mag, init = C.gl_other_sizes_input(n_fft, win, B, T)
    for n_iter in (1, 0):
        _gl_check(mag, init, win, hop, n_fft, n_iter, 'f32 GL {}/{}/{} it={}'.format(n_fft, win, hop, n_iter))


@pytest.mark.parametrize('per_launch', [1, 2, 3])
def test_float32_griffin_lim_second_window(per_launch):
    mag, init = C.gl_second_window_input(per_launch)
    _gl_check(mag, init, 800, 200, 2048, 7, 'f32 GL 800/200 seed {}'.format(per_launch))


@pytest.mark.parametrize('T', C.GL_CHUNK_T)
def test_float32_griffin_lim_chunk_boundaries(T):
    mag, init = C.gl_chunk_input(T)
    _gl_check(mag[None], init, 1102, 275, 2048, 2, 'f32 GL chunk T={}'.format(T))
