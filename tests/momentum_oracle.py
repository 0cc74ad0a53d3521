"""Fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013) restated on the CPU: the reference's loop
(audio/synthesis.py:85-123, oracle.audio_oracle.griffin_lim_v2) with the momentum term

    c_i = stft(istft(|S| angles_i))                      complex64, as in the reference's loop
    mse = mean((|S| - |c_i|)^2)                          of the projection c_i
    t_i = c_i                       (i == 0)
        = c_i + alpha (c_i - c_{i-1})
    angles_{i+1} = t_i / |t_i|      (1 where t_i == 0)

(librosa's ``rebuilt - momentum / (1 + momentum) * tprev`` is t_i / (1 + alpha): the normalisation removes the scale.)
A plain helper module, imported like audio_cases.py: a float64 restatement on the oracle's stft / istft, which IS
griffin_lim_v2 at alpha = 0, and a float32 one on audio_cases.stft32 / istft32 in the style of griffin_lim32.
"""
import os

import numpy as np

import audio_cases as C
from oracle import audio_oracle as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def alpha_of(momentum):
    """the float32 alpha the library makes of a momentum: thousandths, then (float)(v / 1000.0)"""
    return np.float32(min(999, int(round(float(momentum) * 1000.0))) / 1000.0)


def griffin_lim_momentum(spectrogram, win_length, hop_length, n_fft, n_iter, init_phase, momentum=0.0, history=None):
    """float64: (signal float32, mse of the last iteration or None).  momentum == 0 takes griffin_lim_v2's own
    statements, so the two agree bit for bit; with momentum, t and its angle are float64."""
    spectrogram = np.asarray(spectrogram)
    alpha = float(alpha_of(momentum))
    mse = None
    angles = np.exp(2j * np.pi * np.asarray(init_phase, dtype=np.float64))
    mag = np.abs(spectrogram).astype(np.complex128)
    prev = None
    for _ in range(n_iter):
        sig = A.istft(mag * angles, hop_length, win_length)
        c = A.stft(sig, n_fft, hop_length, win_length)
        mse = np.square(np.abs(spectrogram) - np.abs(c)).mean()
        if alpha == 0.0 or prev is None:
            t = c
        else:
            c128 = c.astype(np.complex128)
            t = c128 + alpha * (c128 - prev.astype(np.complex128))
        ang = np.angle(t)
        angles = (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)
        prev = c
        if history is not None:
            history.append(float(mse))
    return A.istft(mag * angles, hop_length, win_length), mse


def griffin_lim_momentum32(mag, win, hop, n_fft, n_iter, init_phase, momentum=0.0):
    """float32 (torch on the CPU, audio_cases.stft32 / istft32), the previous projection kept in complex64."""
    mag = np.abs(np.asarray(mag, dtype=np.float32))
    alpha = alpha_of(momentum)
    u = np.asarray(init_phase, dtype=np.float32).astype(np.float64)
    angles = np.exp(2j * np.pi * u).astype(np.complex64)
    mse, prev = None, None
    for _ in range(n_iter):
        sig = C.istft32(mag * angles, win, hop)
        c = C.stft32(sig[None], n_fft, win, hop)[0].astype(np.complex64)
        mse = float(np.mean(np.square(mag.astype(np.float64) - np.abs(c).astype(np.float64))))
        t = c if (alpha == 0 or prev is None) else (c + alpha * (c - prev)).astype(np.complex64)
        a = np.abs(t)
        angles = np.where(a > 0, t / np.maximum(a, np.float32(1e-37)), np.complex64(1)).astype(np.complex64)
        prev = c
    return C.istft32(mag * angles, win, hop), mse


def shipped_spectrogram(t0=100, t1=400):
    """Frames t0:t1 of the one model output the reference ships (tests/golden/reference_linear_spec_post_215k.npz, a
    normalised linear spectrogram), de-normalised the way inference does it -- mel constants 6.02 / 99.89, power 1.3 --
    and initial phases from default_rng(0): ((1025, t1 - t0) float32 magnitude, (1025, t1 - t0) float32 U[0, 1))."""
    spec = np.load(os.path.join(GOLDEN, 'reference_linear_spec_post_215k.npz'))['linear_spec']
    lin = np.ascontiguousarray(spec[0, :, t0:t1, 0].T)
    mag = A.linear_to_magnitude(lin, 6.02, 99.89, 1.3).astype(np.float32)
    init = np.random.default_rng(0).random(mag.shape).astype(np.float32)
    return mag, init


# the momentum cases of test_gpu_momentum.py, by name: (mag (B, F, T), init, win, hop, n_fft, n_iter, momentum)
def case_per_launch(k, momentum):
    B, T, n_iter, _ = C.GL_PER_LAUNCH[k]
    mag, init = C.gl_per_launch_input(B, T, n_iter)
    return mag, init, 1102, 275, 2048, n_iter, momentum


def case_second_window(per_launch):
    mag, init = C.gl_second_window_input(per_launch)
    return mag, init, 800, 200, 2048, 7, 0.99


def case_other_sizes(k):
    n_fft, win, hop, B, T = C.GL_OTHER_SIZES[k]
    mag, init = C.gl_other_sizes_input(n_fft, win, B, T)
    return mag, init, win, hop, n_fft, 3, 0.99


def case_run_cut(run_len):
    mag, init = C.gl_run_cut_input(run_len)
    return mag[:2], init[:2], 1102, 275, 2048, 4, 0.99


_REF = {}


def reference(key, case):
    """[(waveform, mse) per utterance] of the float64 restatement for a case, computed once per process"""
    if key not in _REF:
        mag, init, win, hop, n_fft, n_iter, momentum = case
        _REF[key] = [griffin_lim_momentum(mag[b], win, hop, n_fft, n_iter, init[b], momentum) for b in range(mag.shape[0])]
    return _REF[key]
