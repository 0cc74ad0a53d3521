"""Inputs of the limiter and true-peak tests, each seeded by its own length so that a row is the same in every batch it appears in.
No GPU, no library."""
import numpy as np

import limiter_oracle as O

SR = 22050
CEILING = 0.5
T = O.TILE


def speech_like(n, amp=0.45, seed=None):
    """bursts of coloured noise at about ``amp``: under CEILING at the default, over it here and there at 0.8 and more"""
    rng = np.random.RandomState(n if seed is None else seed)
    x = rng.randn(n + 2)
    x = (x[2:] + 1.5 * x[1:-1] + x[:-2]) / 3.5
    env = 0.3 + 0.7 * np.abs(np.sin(np.arange(n) * (2 * np.pi / 1500.0) + rng.rand()))
    return (amp * 0.5 * x * env).astype(np.float32)


def quiet(n):
    """a row whose envelope stays under CEILING in both modes"""
    return np.clip(speech_like(n, 0.3), -0.3, 0.3).astype(np.float32)


def with_peaks(n, at, height=0.9):
    """a quiet row with single samples of +-height at the positions ``at`` (those outside 0 .. n - 1 are dropped)"""
    x = quiet(n)
    for k, i in enumerate(at):
        if 0 <= i < n:
            x[i] = height * (1 if k % 2 == 0 else -1) * (1.0 + 0.1 * k)
    return x


def kitchen(n, L):
    """one row with everything the gain rule distinguishes, placed by the look-ahead L and the tile edge: peaks at 0 and n - 1, two
    closer than L, two closer than 2 L but not L, a plateau of equal samples over the ceiling, peaks either side of every tile
    edge, and quiet stretches longer than the tile plus its halo in between where the row is long enough"""
    at = [0, n - 1, 300, 300 + max(1, L - 1), 700 + 3 * L, 700 + 3 * L + max(2, 2 * L - 1)]
    for edge in range(T, n, T):
        at += [edge - 1, edge, edge + L + 1]
    x = with_peaks(n, at)
    lo = min(n, 1200 + 6 * L)
    x[lo:min(n, lo + 40)] = 0.75          # the plateau
    return x


def specials(n):
    """NaN, +-Inf and -0.0 among samples over the ceiling"""
    x = speech_like(n, 1.6)
    for i, v in ((3, np.nan), (n // 3, np.inf), (n // 3 + 2, -np.inf), (n // 2, -0.0), (n - 2, np.nan)):
        x[i] = v
    return x


def padded(rows, fill):
    """(X (B, N) float32 with ``fill`` behind every row, the lengths int32)"""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    X = np.full((len(rows), int(lens.max())), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        X[b, :len(r)] = r
    return X, lens


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tones(f_max, n_freq=45, n_phase=33, n=400):
    """(f, phase, x float32 (n,), the exact 4x points (n, 4)) for tones of amplitude 1 up to f_max (in units of the sampling rate)"""
    t = np.arange(n)
    for f in np.linspace(0.01, f_max, n_freq):
        for k in range(n_phase):
            ph = 2 * np.pi * k / n_phase
            yield f, ph, np.sin(2 * np.pi * f * t + ph).astype(np.float32), np.stack([np.sin(2 * np.pi * f * (t + p / 4.0) + ph) for p in range(4)], 1)
