"""Oracle of the speaking-rate feature: a from-scratch numpy restatement, in float64, of what the reference's time_stretch
(audio/effects.py:46-88) hands to Griffin-Lim -- librosa 0.6 phase_vocoder(stft, rate) followed by np.abs.

Two forms.  `blend` is what the library computes: the vocoder's magnitude interpolation alone, rounded once to float32.
`vocoder_abs` is the whole path: the same interpolation, the accumulated phases, the product cast to complex64 as the
vocoder's output array is, and np.abs of that.  The phase has modulus one, so the two differ by rounding only:
2^-24 (complex64 cast) + 2^-23 (float32 abs) + 2^-24 (the blend's own rounding) = 2^-22 relative."""
import numpy as np

RATE_MIN, RATE_MAX = 0.25, 4.0
BOUND_FULL_PATH = 2.0 ** -22


def time_steps(n, rate):
    """the times, in input frames, of the output frames: 0, rate, 2 rate, ... below n"""
    return np.arange(0, n, rate, dtype=np.float64)


def stretched_frames(n, rate):
    return len(time_steps(n, rate))


def _weights(n, rate):
    s = time_steps(n, rate)
    i = s.astype(np.int64)          # (s >= 0: truncation is the floor)
    a = s - np.floor(s)
    return i, a


def blend_f64(x, rate):
    """x (F, n) -> (F, n_out) float64: frame k is (1 - a) x[:, i] + a x[:, i + 1] with s = k rate, i = int(s), a = s - i;
    columns n and n + 1 are zeros (the vocoder pads its input by two).  Every product and the sum are separate float64
    operations; 0 * NaN stays NaN."""
    x = np.asarray(x)
    F, n = x.shape
    xp = np.zeros((F, n + 2), np.float64)
    xp[:, :n] = x
    i, a = _weights(n, rate)
    with np.errstate(invalid='ignore'):
        return (1.0 - a)[None, :] * xp[:, i] + a[None, :] * xp[:, i + 1]


def blend(x, rate):
    """the round-once blend: blend_f64 as float32"""
    with np.errstate(over='ignore'):
        return blend_f64(x, rate).astype(np.float32)


def blend_batch(x, rate, n_frames=None, T_out=None):
    """x (B, F, T) float32, n_frames: B lengths or None (all T) -> (B, F, T_out) float32: utterance b is blend() of its
    first n_frames[b] columns followed by zeros; T_out None: the longest stretched length"""
    x = np.asarray(x, dtype=np.float32)
    B, F, T = x.shape
    nf = [T] * B if n_frames is None else [int(v) for v in n_frames]
    longest = max(stretched_frames(n, rate) for n in nf)
    T_out = longest if T_out is None else T_out
    assert T_out >= longest
    out = np.zeros((B, F, T_out), np.float32)
    for b, n in enumerate(nf):
        y = blend(x[b, :, :n], rate)
        out[b, :, :y.shape[1]] = y
    return out


def vocoder_abs(mag, phase, rate, hop_length=None):
    """The whole path on an STFT given as magnitudes (F, n) float32 and phases (F, n) in radians: per output frame the
    interpolated magnitude times exp(1j accumulated phase) is stored as complex64, and the result is np.abs of that array
    (float32).  The phase accumulator starts at the phases of frame 0 and advances by the expected advance of each bin
    plus the wrapped deviation between the two neighbouring input frames."""
    mag = np.asarray(mag, dtype=np.float32)
    F, n = mag.shape
    n_fft = 2 * (F - 1)
    hop = n_fft // 4 if hop_length is None else hop_length
    magp = np.zeros((F, n + 2), np.float64)
    magp[:, :n] = mag
    php = np.zeros((F, n + 2), np.float64)     # (the angle of the zero padding is 0)
    php[:, :n] = phase
    expected = np.linspace(0.0, np.pi * hop, F)
    acc = php[:, 0].copy()
    i, a = _weights(n, rate)
    out = np.zeros((F, len(i)), np.complex64)
    for k in range(len(i)):
        m = (1.0 - a[k]) * magp[:, i[k]] + a[k] * magp[:, i[k] + 1]
        out[:, k] = m * np.exp(1j * acc)
        d = php[:, i[k] + 1] - php[:, i[k]] - expected
        d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        acc += expected + d
    return np.abs(out)


def stretched_lengths(n, rate, T_out, min_frames):
    """the lengths a call with end-of-speech stopping reports: min(T', max(min_frames, ceil(n / rate)))"""
    return np.array([min(T_out, max(min_frames, stretched_frames(int(v), rate))) for v in n], np.int32)
