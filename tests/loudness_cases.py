"""The cases of the loudness tests, shared by the host tests (tests/test_loudness_host.py) and the GPU tests
(tests/test_gpu_loudness*.py).  Every input is seeded by its own length and sampling rate, so an utterance is the same array in
any batch."""
import numpy as np

import loudness_oracle as O

SR = 22050


def lengths_22050():
    """no block, one block, a few, and both sides of a segment edge behind eleven steps"""
    s, c = O.step(SR), O.segment(SR)
    return [4 * s - 1, 4 * s, 5 * s + 17, 11 * s + c - 1, 11 * s + c]


# (sampling rate, samples): 22 050 Hz has unequal segments (7 x 276 + 273), 16 000 Hz equal ones
MEASURE = [(SR, n) for n in lengths_22050()] + [(16000, 7 * 1600 + 3), (48000, 5 * 4800 + 1)]
RAGGED = lengths_22050()          # one call, rows of the longest
TONE_RATES = [48000, 44100, 22050, 16000, 8000]


def speech_like(n, sr, amplitude=0.1):
    """(n,) float32: noise under a slow envelope plus a tone -- levels well above float32's subnormals"""
    rng = np.random.default_rng([n, sr])
    t = np.arange(n, dtype=np.float64) / sr
    envelope = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.1 * t + rng.uniform(0, 6.28))
    x = envelope * rng.standard_normal(n) * 0.5 + 0.7 * np.sin(2.0 * np.pi * 211.0 * t)
    return (amplitude * x).astype(np.float32)


def sine(sr, seconds=2.0, hz=997.0, amplitude=1.0):
    t = np.arange(int(round(seconds * sr)), dtype=np.float64) / sr
    return (amplitude * np.sin(2.0 * np.pi * hz * t)).astype(np.float32)


def tone_at(level_lufs, seconds, sr, hz=997.0):
    """a 997 Hz tone that reads about ``level_lufs`` (a full-scale one reads -3.01)"""
    return sine(sr, seconds, hz, 10.0 ** ((level_lufs + 3.0103) / 20.0))


def relative_gate_signal(sr=16000):
    """1 s at -36, 3 s at -23, 1 s at -36 LUFS: the relative gate drops the quiet blocks"""
    return np.concatenate([tone_at(-36.0, 1.0, sr), tone_at(-23.0, 3.0, sr), tone_at(-36.0, 1.0, sr)])


def absolute_gate_signal(sr=16000):
    """1 s of zeros, 2 s at -23 LUFS, 1 s of zeros: the absolute gate drops the silent blocks"""
    return np.concatenate([np.zeros(sr, np.float32), tone_at(-23.0, 2.0, sr), np.zeros(sr, np.float32)])


def all_cases():
    """(name, sampling rate, waveform) of every input the tests use"""
    out = [('speech_%d_%d' % (sr, n), sr, speech_like(n, sr)) for sr, n in MEASURE]
    out += [('sine_%d' % sr, sr, sine(sr)) for sr in TONE_RATES]
    out += [('relative_gate', 16000, relative_gate_signal()), ('absolute_gate', 16000, absolute_gate_signal())]
    return out


def padded(rows, fill=np.nan):
    """the utterances as rows of the longest, ``fill`` behind each -> (B, N) float32, lengths int32"""
    N = max(len(r) for r in rows)
    out = np.full((len(rows), N), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32)
