"""Inputs of the estimated-initial-phase tests (a plain helper module, imported like stretch_cases.py): the magnitudes the
kernels of csrc/phase_init.hip are held to tests/phase_oracle.py on, by name, and the fixture slice of the quality statement.
The shapes are the smallest at which the kernels can go wrong: one bin count per row width the audio surface has an edge at
(129, 1025, 2049 bins), frame counts at both sides of the kernel's chunk length, and ragged batches."""
import numpy as np

import momentum_oracle as M

HOP = {256: 64, 2048: 275, 4096: 512}
KINDS = ['random', 'quantised', 'ramp-up', 'ramp-down', 'zeros', 'chirp', 'nan-inf', 'fixture']


def frame_counts(n_fft, chunk):
    """the T of the bit-for-bit tests at an n_fft, for a kernel that cuts time into chunks of `chunk` frames"""
    if n_fft == 256:
        return [1, 2, 41]
    if n_fft == 4096:
        return [5]
    return sorted({9, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 31, 32, 33, 67})


def fixture_magnitudes(t0=100, t1=260):
    """frames t0:t1 of the shipped spectrogram, de-normalised as inference does it: (1025, t1 - t0) float32"""
    return M.shipped_spectrogram(t0, t1)[0]


def magnitudes(kind, n_fft, T, seed=0):
    """(F, T) float32"""
    F = 1 + n_fft // 2
    rng = np.random.default_rng([seed, n_fft, T, KINDS.index(kind)])
    k = np.arange(F, dtype=np.float32)[:, None]
    if kind == 'random':            # peaks everywhere
        return rng.random((F, T)).astype(np.float32)
    if kind == 'quantised':         # ties everywhere
        return rng.integers(0, 4, (F, T)).astype(np.float32)
    if kind == 'ramp-up':           # one peak at F - 2, owned by walks of length F; the frames differ in scale
        m = np.repeat(k, T, axis=1) * (1.0 + np.arange(T, dtype=np.float32)[None, :])
        m[F - 1] = 0.0
        return m.astype(np.float32)
    if kind == 'ramp-down':         # one peak at 1
        m = np.repeat((F - k), T, axis=1) + np.arange(T, dtype=np.float32)[None, :]
        m[0] = 0.0
        return m.astype(np.float32)
    if kind == 'zeros':
        return np.zeros((F, T), np.float32)
    if kind == 'chirp':             # a peak that moves a bin per frame over a floor of small noise: owners change
        m = (rng.random((F, T)) * 1e-3).astype(np.float32)
        for t in range(T):
            c = 3 + (5 * n_fft // 256 + t) % (F - 6)
            m[c - 2:c + 3, t] += np.array([0.1, 0.5, 1.0, 0.6, 0.2], np.float32)
        return m
    if kind == 'nan-inf':           # random, with columns that hold NaN and +Inf bins (isolated, adjacent, at both edges)
        m = rng.random((F, T)).astype(np.float32)
        t = T // 2
        m[[0, 7, 8, F // 2, F - 1], t] = np.nan
        m[[3, 20, 21, F - 3], t] = np.inf
        if T > 1:
            m[5, T - 1] = np.inf
            m[F - 2, 0] = np.nan
        return m
    if kind == 'fixture':           # |stft| of real speech as the network predicts it; other sizes: its low bins, tiled in time
        src = fixture_magnitudes()
        reps = -(-T // src.shape[1])
        rows = np.tile(src, (-(-F // src.shape[0]), reps))
        return np.ascontiguousarray(rows[:F, :T])
    raise KeyError(kind)


def ragged_lengths(T):
    return np.array([T, 1, max(1, T // 2)], np.int32)


def ragged_batch(n_fft, T, seed=3):
    """(mag (3, F, T) with NaN behind every utterance's end, n_frames): three kinds side by side"""
    n = ragged_lengths(T)
    mag = np.stack([magnitudes(kind, n_fft, T, seed) for kind in ('random', 'chirp', 'quantised')])
    for b in range(3):
        mag[b, :, n[b]:] = np.nan
    return mag, n
