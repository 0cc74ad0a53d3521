"""Inputs, shape tables and a float32 restatement for the audio kernels' per-slice tests (a plain helper module, imported
like parity.py and trim_oracle.py).

The GPU tests (test_gpu_analysis.py, test_gpu_audio.py, test_gpu_edge_cases.py) hold every bin, frame, channel and hop
segment to the project's existing bounds (1e-5 for the analysis side, 1e-4 max(1, n_iter) for Griffin-Lim) against the
float64 oracle.  test_audio_bounds_host.py runs the float32 restatement below -- torch.stft / torch.fft.irfft on the CPU,
a float32 overlap-add -- against the same oracle on the SAME inputs and asserts that plain float32 arithmetic stays
within a quarter of every such bound: the inputs neither flatter the bound nor defeat it.
"""
import numpy as np

from oracle import audio_oracle as A

ANALYSIS_TOL = 1e-5          # complex STFT, |S| ** p and mel: per utterance, bin / channel, frame and element
GL_TOL = 1e-4                # Griffin-Lim waveform: times max(1, n_iter), per utterance and per hop segment
HOST_MARGIN = 0.25           # the float32 restatement must stay within this fraction of a bound

STFT_AXES = {'utt': 0, 'bin': 1, 'frame': 2}       # (B, F, frames[, re / im])
MEL_AXES = {'utt': 0, 'chan': 1, 'frame': 2}       # (B, n_mels, frames)


def gl_tol(n_iter):
    return GL_TOL * max(1, n_iter)


# ----------------------------------------------------------------------------------------------- signals
def tone_noise(rng, n, b=0, sr=22050.0):
    """the suite's sine-plus-noise signal; the tone moves with the utterance index"""
    t = np.arange(n) / sr
    return (0.3 * np.sin(2 * np.pi * (220 + 40 * b) * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def broadband(rng, n, b=0, sr=22050.0):
    """harmonics of a fundamental that moves with the utterance index (1 / k amplitudes, up to the Nyquist frequency), a
    -30 dB noise floor, a DC offset and a component AT the Nyquist frequency: every bin, the first and the last one
    included, carries signal"""
    t = np.arange(n) / sr
    f0 = 110.0 + 23.0 * b
    y = np.zeros(n)
    for k in range(1, int(sr / 2 / f0)):
        y += np.sin(2 * np.pi * f0 * k * t + 0.7 * k) / k
    y *= 0.2
    y += 0.05 + 0.05 * np.cos(np.pi * np.arange(n)) + 10.0 ** (-30 / 20.0) * rng.standard_normal(n)
    return y.astype(np.float32)


SIGNALS = {'tone': tone_noise, 'broadband': broadband}


def signals(kind, seed, B, n):
    """(B, n) float32, a different signal per utterance (a wrong utterance stride cannot match by accident)"""
    rng = np.random.default_rng(seed)
    return np.stack([SIGNALS[kind](rng, n, b) for b in range(B)])


def synth_mag(rng, B, T, n_fft=2048, hop=275, win=1102):
    """magnitude spectrograms of band-limited noise + tones, (B, F, T) float32 (the Griffin-Lim tests' input)"""
    out = []
    for b in range(B):
        n = hop * (T - 1)
        t = np.arange(n) / 22050.0
        y = 0.3 * np.sin(2 * np.pi * (220 + 40 * b) * t) + 0.1 * rng.standard_normal(n)
        out.append(np.abs(A.stft(y.astype(np.float32), n_fft, hop, win)).astype(np.float32))
    return np.stack(out)


def power4_mag(rng, shape):
    """random magnitudes with a long tail, as the other-sizes Griffin-Lim tests use them"""
    return ((rng.random(shape) ** 4) * 10).astype(np.float32)


# ----------------------------------------------------------------------------------------------- analysis tables
# (n_fft, win, hop): the n_fft 2048 kernel (stft_kernel) with the model's window, the 16 kHz one, a full and an odd window;
# the general kernels (glg_stft_kernel) at their four other sizes
STFT_CONFIGS = [(2048, 1102, 275), (2048, 800, 200), (2048, 2048, 512), (2048, 1103, 275),
                (256, 200, 50), (512, 400, 100), (1024, 800, 200), (4096, 2400, 600)]
# the eight shape sets the bounds were first measured on, (n_fft, win, hop, n)
MEASURED_SHAPES = [(2048, 1102, 275, 8250), (2048, 1102, 275, 1025), (2048, 1103, 275, 9001), (2048, 2048, 512, 20011),
                   (1024, 800, 200, 7777), (4096, 2400, 600, 30001), (256, 200, 50, 2345), (512, 400, 100, 257)]


def _analysis_cases():
    """(n_fft, win, hop, n, B): per configuration the shortest legal length (n_fft / 2 + 1: every frame reflects on both
    sides), a length = 1 (mod hop) just above it and below n_fft, a length = hop - 1 (mod hop) above n_fft, an exact
    multiple of the hop; B = 1, 3 and 9 go round the lengths.  One long case: 3001 frames at hop 50."""
    cases = []
    for i, (n_fft, win, hop) in enumerate(STFT_CONFIGS):
        half = n_fft // 2
        lengths = [half + 1,
                   hop * (-(-(half + 2) // hop)) + 1,
                   hop * (-(-n_fft // hop) + 17) + hop - 1,
                   hop * 37]
        assert half < lengths[1] < n_fft < lengths[2], (n_fft, hop, lengths)
        for j, n in enumerate(lengths):
            cases.append((n_fft, win, hop, n, (1, 3, 9)[(i + j) % 3]))
    for k, (n_fft, win, hop, n) in enumerate(MEASURED_SHAPES):
        cases.append((n_fft, win, hop, n, (3, 1)[k % 2]))
    cases.append((256, 200, 50, 50 * 3000 + 7, 2))
    return cases


ANALYSIS_CASES = _analysis_cases()
POWERS = (1.0, 2.0, 1.3)
# (sr, n_fft, n_mels, fmin, fmax); fmax None: sr / 2 (the C entry point takes fmax <= 0 for it)
MEL_CONFIGS = [(22050, 2048, 80, 0.0, 8000.0), (16000, 1024, 40, 50.0, 7600.0), (22050, 512, 128, 0.0, None),
               (22050, 4096, 1, 0.0, 8000.0)]
MEL_FRAMES = (1, 33, 1000)
MEL_BATCHES = (1, 3)


def mel_input(cfg_index, n_frames, B):
    """(B, F, n_frames) float32 non-negative 'linear spectrogram' of a mel case, different per utterance"""
    n_fft = MEL_CONFIGS[cfg_index][1]
    rng = np.random.default_rng(1000 * cfg_index + 10 * n_frames + B)
    return power4_mag(rng, (B, 1 + n_fft // 2, n_frames))


def ref_stft(y, n_fft, win, hop):
    """float64 oracle of a batch, complex128 (B, F, frames): NOT the oracle's default complex64 cast"""
    return np.stack([A.stft(u, n_fft, hop, win, dtype=np.complex128) for u in y])


def as_real(z):
    """complex (...,) -> float (..., 2): real and imaginary part as a trailing axis, so that a slice's error is the
    complex one"""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], axis=-1)


# ----------------------------------------------------------------------------------------------- Griffin-Lim tables
# Every table below is (what the GPU test of that name feeds its kernel, by the same generator and seed).
GL_FEW = [(1, 12, 0), (2, 12, 1), (2, 40, 1), (1, 70, 3)]                                   # (B, T, n_iter)
GL_PER_LAUNCH = [(2, 40, 6, False), (1, 70, 7, True), (3, 151, 5, True), (2, 9, 4, False)]   # (B, T, n_iter, want_mse)
GL_RUN_LENS = [8, 16, 40, 104, 296]
GL_RUN_CUT_FORMS = [(1, 2, True), (3, 4, False)]                                            # (per_launch, n_iter, want_mse)
GL_OTHER_SIZES = [(1024, 800, 200, 3, 60), (4096, 2400, 600, 2, 40), (512, 512, 128, 2, 50), (256, 200, 50, 1, 45),
                  (2048, 1200, 300, 2, 40), (2048, 800, 200, 3, 60), (2048, 800, 200, 1, 260), (2048, 2048, 512, 1, 30)]
GL_CHUNK_T = [5, 6, 31, 32, 33, 64, 65]


def gl_few_input(B, T, n_iter):
    rng = np.random.default_rng(10 * T + n_iter)
    mag = synth_mag(rng, B, T)
    return mag, rng.random(mag.shape).astype(np.float32)


def gl_per_launch_input(B, T, n_iter):
    rng = np.random.default_rng(1000 * T + n_iter)
    mag = synth_mag(rng, B, T)
    return mag, rng.random(mag.shape).astype(np.float32)


def gl_run_cut_input(run_len):
    rng = np.random.default_rng(run_len)
    mag = synth_mag(rng, 5, 151)
    return mag, rng.random(mag.shape).astype(np.float32)


def gl_other_sizes_input(n_fft, win, B, T):
    rng = np.random.default_rng(n_fft + win)
    F = 1 + n_fft // 2
    mag = power4_mag(rng, (B, F, T))
    return mag, rng.random((B, F, T)).astype(np.float32)


def gl_second_window_input(per_launch):
    rng = np.random.default_rng(800 + per_launch)
    mag = power4_mag(rng, (3, 1025, 150))
    return mag, rng.random((3, 1025, 150)).astype(np.float32)


def gl_chunk_input(T, hop=275, win=1102, n_fft=2048):
    rng = np.random.default_rng(T)
    n = hop * (T - 1)
    y = (0.2 * np.sin(2 * np.pi * 300 * np.arange(n) / 22050) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    mag = np.abs(A.stft(y, n_fft, hop, win)).astype(np.float32)
    return mag, rng.random((1, 1025, T)).astype(np.float32)


# ----------------------------------------------------------------------------------------------- float32 restatement
def _window32(win):
    import torch
    return torch.from_numpy(A.hann_periodic(win).astype(np.float32))


def stft32(y, n_fft, win, hop):
    """librosa.stft in float32: torch.stft on the CPU (centre / reflect padding, the periodic hann rounded to float32 and
    padded to n_fft).  y (B, n) float32 -> complex64 (B, F, frames)."""
    import torch
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    S = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=_window32(win), center=True, pad_mode='reflect',
                   normalized=False, onesided=True, return_complex=True)
    return S.numpy()


def magnitude32(S, power):
    m = np.abs(S.astype(np.complex64)).astype(np.float32)
    return m if power == 1.0 else (m * m if power == 2.0 else np.power(m, np.float32(power)))


def mel32(lin, sr, n_fft, n_mels, fmin, fmax):
    """float32 filter bank times float32 spectrogram, float32 accumulation.  lin (B, F, frames) -> (B, n_mels, frames)."""
    import torch
    bank = torch.from_numpy(A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(np.float32))
    return torch.matmul(bank, torch.from_numpy(np.ascontiguousarray(lin, dtype=np.float32))).numpy()


def istft32(spec, win, hop):
    """librosa.istft in float32: torch.fft.irfft of complex64 frames, float32 synthesis window, frames overlap-added one
    after the other into a float32 buffer, divided by the oracle's float32 window sum.  spec (F, frames) -> (hop (frames - 1),)"""
    import torch
    n_fft = 2 * (spec.shape[0] - 1)
    T = spec.shape[1]
    frames = torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(spec.T, dtype=np.complex64)), n=n_fft, dim=1)
    lpad = (n_fft - win) // 2
    frames = (frames[:, lpad:lpad + win] * _window32(win)[None, :]).numpy()
    y = np.zeros(n_fft + hop * (T - 1), np.float32)
    for t in range(T):
        y[t * hop + lpad:t * hop + lpad + win] += frames[t]
    wss = A.window_sumsquare(T, hop, win, n_fft, dtype=np.float32)
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:-(n_fft // 2)]


def griffin_lim32(mag, win, hop, n_fft, n_iter, init_phase):
    """griffin_lim_v2 of one utterance in float32 from the given initial phases -> (waveform float32, mse of the last
    iteration or None)."""
    mag = np.abs(np.asarray(mag, dtype=np.float32))
    u = np.asarray(init_phase, dtype=np.float32).astype(np.float64)
    angles = np.exp(2j * np.pi * u).astype(np.complex64)
    mse = None
    for _ in range(n_iter):
        sig = istft32(mag * angles, win, hop)
        est = stft32(sig[None], n_fft, win, hop)[0]
        a = np.abs(est)
        angles = np.where(a > 0, est / np.maximum(a, np.float32(1e-37)), np.complex64(1)).astype(np.complex64)
        mse = float(np.mean(np.square(mag.astype(np.float64) - a.astype(np.float64))))
    return istft32(mag * angles, win, hop), mse
