"""Inputs of the equaliser tests, each seeded by its own length so that a row is the same in every batch it appears in, and the
cascades they run through.  No GPU, no library."""
import numpy as np

import equalizer_oracle as O

SR = 22050
FILL = np.float32(-7.25)        # what stands behind every row of a ragged batch, and must come back untouched


def speech_like(n, amp=0.45, seed=None):
    """bursts of coloured noise at about ``amp``"""
    rng = np.random.RandomState(n if seed is None else seed)
    x = rng.randn(n + 2)
    x = (x[2:] + 1.5 * x[1:-1] + x[:-2]) / 3.5
    env = 0.3 + 0.7 * np.abs(np.sin(np.arange(n) * (2 * np.pi / 1500.0) + rng.rand()))
    return (amp * 0.5 * x * env).astype(np.float32)


def cascade(S):
    """S sections that differ from each other: the profiles and a few designs at 22050 Hz, cut or repeated to S"""
    pool = np.concatenate([O.profile('telephony', SR), O.profile('small-speaker', SR)[2:], O.profile('warm', SR),
                           O.design(O.PEAK, SR, 900.0, 4.0, -6.0)[None]])
    assert len(pool) == 8
    return np.ascontiguousarray(pool[:S])


def specials(n):
    """-0.0 and float32 denormals among the samples, then an Inf and a NaN two thirds in: what follows them is NaN"""
    x = speech_like(n, seed=n + 3)
    tiny = np.float32(1e-45)
    for i, v in ((0, -0.0), (1, tiny), (2, -tiny), (n // 3, np.float32(1.1e-39)), (n // 3 + 1, -0.0)):
        if i < n:
            x[i] = v
    if n > 8:
        x[2 * n // 3] = np.inf
        x[2 * n // 3 + 2] = np.nan
    return x


def denormal(n):
    """a row of float32 denormals and zeros alone"""
    rng = np.random.RandomState(n + 11)
    return (rng.randint(-40, 41, n) * np.float32(1e-45)).astype(np.float32)


def padded(rows, N=None, fill=FILL):
    """(X (B, N) float32 with ``fill`` behind every row, the lengths int32)"""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    X = np.full((len(rows), int(lens.max()) if N is None else N), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        X[b, :len(r)] = r
    return X, lens


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """bit for bit on every finite value, NaN where NaN is wanted (payloads are not compared)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
