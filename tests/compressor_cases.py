"""Inputs and parameter sets of the compressor tests, each row seeded by its own length so that it is the same in every batch it
appears in, the bound the output is held to, and the condition under which the records are exact.  No GPU, no library."""
import numpy as np

import compressor_oracle as O
from equalizer_cases import FILL, bits, padded, same, speech_like   # noqa: F401

SR = 22050
INF = float('inf')
# (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db) at SR: every path of the gain computer and of the detector
SETS = {
    'speech': O.PROFILES['speech'],
    'soft': (-30.0, 4.0, 12.0, 1.0, 50.0, 6.0),            # a wide knee, make-up
    'hard': (-20.0, INF, 0.0, 0.0, 0.0, 0.0),              # slope 0, knee 0, attack 0, release 0: e = |x|
    'unity': (-20.0, 1.0, 6.0, 5.0, 100.0, 0.0),           # slope 1, make-up 0: the identity
    'instant_attack': (-25.0, 2.0, 0.0, 0.0, 80.0, -3.0),  # attack 0, knee 0, a negative make-up
    'no_release': (-25.0, 8.0, 6.0, 2.0, 0.0, 2.0),        # release 0
    'slow': (-35.0, 3.0, 6.0, 20.0, 2000.0, 0.0),          # the longest times of the measured range: states cross many segments
}


def params(name_or_tuple, sr=SR):
    t = SETS[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    return O.params(*t, sr=sr)


def as_engine(p):
    """the oracle's parameters as ``Engine.compress`` takes coefficients made elsewhere"""
    return ('params', tuple(p))


def burst(n, at=40, length=300):
    """a loud burst near the front, then silence (exact zeros) with two faint clicks far behind: the state it leaves is carried
    across every segment, and across a tile where n is beyond one"""
    x = np.zeros(n, np.float32)
    hi = min(n, at + length)
    if hi > at:
        x[at:hi] = 0.9 * speech_like(hi - at, amp=1.8, seed=n + 1)
    for p in (n // 2, n - 3):
        if p > hi:
            x[p] = np.float32(1e-4)
    return x


def specials(n):
    """-0.0, float32 denormals, an Inf and a NaN among speech-like samples; a NaN and an Inf right at the front too"""
    x = speech_like(n, seed=n + 3)
    tiny = np.float32(1e-45)
    for i, v in ((0, np.nan), (1, -0.0), (2, tiny), (3, -tiny), (4, np.inf), (n // 3, np.float32(1.1e-39)), (n // 3 + 1, -0.0),
                 (2 * n // 3, -np.inf), (2 * n // 3 + 2, np.nan), (n - 1, 0.0)):
        if 0 <= i < n:
            x[i] = v
    return x


def denormal(n):
    """a row of float32 denormals and zeros alone"""
    rng = np.random.RandomState(n + 11)
    return (rng.randint(-40, 41, n) * np.float32(1e-45)).astype(np.float32)


def two_level(sr, lo_db, hi_db, seconds=(0.5, 0.5, 0.5), f=1000.0):
    """a tone at ``lo_db``, then ``hi_db``, then ``lo_db`` again (peak levels re full scale), and the two seams"""
    n = [int(round(s * sr)) for s in seconds]
    t = np.arange(sum(n)) / float(sr)
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for k, db in zip(n, (lo_db, hi_db, lo_db))])
    return (amp * np.sin(2 * np.pi * f * t)).astype(np.float32), n[0], n[0] + n[1]


# ---- what the output is held to
def bound(y):
    """2^-24 |y| (the one rounding to float32) + 2^-40 |y| (the device's log10 and pow against numpy's) + 2^-150"""
    a = np.abs(np.asarray(y, np.float64))
    return 2.0 ** -24 * a + 2.0 ** -40 * a + 2.0 ** -150


def exact_positions(res):
    """where the output is held bit for bit: NaN, Inf, zero and identity positions of the oracle's row"""
    y = res.y
    return res.identity | ~np.isfinite(y) | (y == 0)


def held(got, res):
    """-> (every exact position has the oracle's bits, the largest |got - y| / bound elsewhere)"""
    got = np.asarray(got, np.float32)
    exact = exact_positions(res)
    ok = same(got[exact], res.out[exact])
    rest = ~exact
    if not rest.any():
        return ok, 0.0
    with np.errstate(all='ignore'):
        err = np.abs(got[rest].astype(np.float64) - res.y[rest]) / bound(res.y[rest])
    return ok, float(np.nan_to_num(err, nan=np.inf).max())


def clear_of_the_knee(res, p, margin=1e-9):
    """every level of the row stays ``margin`` dB clear of the knee's lower edge T - W / 2, where r leaves 0: then ``reduced`` does
    not depend on the last bits of log10"""
    L = O.level(res.envelope)
    L = L[np.isfinite(L)]
    return bool(np.all(np.abs(L - (p.threshold_db - p.knee_db / 2.0)) > margin))


def same_doubles(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64))
