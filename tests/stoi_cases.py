"""The inputs of the STOI tests (tests/test_stoi_host.py, tests/test_gpu_stoi*.py): a speech-like signal at 10 kHz, degraded
copies of it, and rows built frame by frame so that a chosen number of frames is kept.  Every row is made once (lru_cache) and
handed out read-only; so is its oracle."""
import functools

import numpy as np

import stoi_oracle as S

SR = 10000
GROUP = 4          # STOI_GROUP (csrc/stoi_plan.h): the kept frames of an envelope workgroup
SEG_CHUNK = 64     # STOI_SEG_CHUNK: the segments of a segment workgroup
SNRS = (30, 20, 10, 0, -10)
N_SEG = S.N         # frames of a segment


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def speech(n=20000, seed=0, floor_db=None):
    """29 harmonics (amplitude 1 / h, all from phase 0) of an F0 of 120 +/- 20 Hz (a 1 Hz vibrato), amplitude modulation
    clip(sin(2 pi 3.1 t), 0)^2 (0.3 + 0.7 |sin(2 pi 0.37 t)|): bursts with silence between them.
    ``floor_db``: white noise at that level under the modulated harmonics' RMS, gated by the same modulation -- energy in every
    band of every kept frame, which the value bound needs."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / float(SR)
    phase = 2 * np.pi * np.cumsum(120.0 + 20.0 * np.sin(2 * np.pi * 1.0 * t)) / SR
    x = np.zeros(n)
    for h in range(1, 30):
        x += np.sin(h * phase) / h
    am = np.clip(np.sin(2 * np.pi * 3.1 * t), 0, None) ** 2 * (0.3 + 0.7 * np.abs(np.sin(2 * np.pi * 0.37 * t)))
    if floor_db is not None:
        x = x + rng.standard_normal(n) * np.sqrt((x ** 2).mean()) * 10.0 ** (floor_db / 20.0)
    return _frozen((0.3 * am * x).astype(np.float32))


@functools.lru_cache(maxsize=None)
def noise(n, seed):
    return _frozen(np.random.default_rng(seed).standard_normal(n))


def degraded(x, snr_db, seed=7):
    """``x`` plus white noise at ``snr_db`` under its power"""
    x64 = np.asarray(x, np.float64)
    g = np.sqrt((x64 ** 2).mean() / 10.0 ** (snr_db / 10.0))
    return (x64 + g * noise(len(x), seed)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loud_quiet(pattern, seed=0, tail=0):
    """A row whose frame m is loud where ``pattern[m]`` is '1' and silent (exact zeros) elsewhere, and its degraded copy: noise
    bursts of 128 samples, burst h loud iff frame h - 1 or h is marked.  A frame that shares one burst with a marked frame is
    kept as well (half its samples are loud), so the count of kept frames is the oracle's to say (``pattern_with_kept``); a
    frame of two silent bursts is exact zeros.  The compaction joins frames that were never neighbours.  ``tail``: samples
    behind the last frame (< 128: no frame more)."""
    F = len(pattern)
    halves = np.zeros(F + 1, bool)
    for m, c in enumerate(pattern):
        if c == '1':
            halves[m] = halves[m + 1] = True
    rng = np.random.default_rng(50 + seed)
    n = (F + 1) * 128 + tail
    gain = np.repeat(np.where(halves, 1.0, 0.0) * rng.uniform(0.5, 1.0, F + 1), 128)
    x = np.zeros(n)
    x[:(F + 1) * 128] = gain * rng.standard_normal((F + 1) * 128) * 0.1
    ref = x.astype(np.float32)
    deg = (x + 0.03 * rng.standard_normal(n) * (gain > 0)).astype(np.float32)
    return _frozen(ref), _frozen(deg)


def runs(kept, lead=0, gap_at=None, gap=0, trail=0):
    """a pattern of ``kept`` marked frames: ``lead`` silent frames in front, ``gap`` silent frames behind the first ``gap_at``
    marked ones, ``trail`` silent frames at the end."""
    body = '1' * kept if gap_at is None else '1' * gap_at + '0' * gap + '1' * (kept - gap_at)
    return '0' * lead + body + '0' * trail


@functools.lru_cache(maxsize=None)
def oracle(key, extended):
    """the oracle of a named row (``row``), once"""
    ref, deg = row(key)
    return S.stoi(ref, deg, extended)


@functools.lru_cache(maxsize=None)
def row(key):
    """(ref, deg) float32 of a named row"""
    kind = key[0]
    if kind == 'speech':            # ('speech', snr_db)
        x = speech(floor_db=-30.0)
        return x, _frozen(degraded(x, key[1]))
    if kind == 'pattern':           # ('pattern', pattern, seed)
        return loud_quiet(key[1], key[2])
    if kind == 'cut':               # ('cut', n): the speech row cut to n samples
        x = speech(floor_db=-30.0)[:key[1]]
        return _frozen(x.copy()), _frozen(degraded(x, 10))
    raise KeyError(key)


def pattern_with_kept(kept, lead=0, gap_at=None, gap=0, trail=0, seed=0):
    """the key of a loud / quiet row that keeps exactly ``kept`` frames (checked on the oracle), silence placed as asked"""
    for marked in range(max(kept - 3, 1), kept + 1):
        key = ('pattern', runs(marked, lead, gap_at, gap, trail), seed)
        ref, _ = row(key)
        if len(S.kept_frames(S.energies(ref))) == kept:
            return key
    raise AssertionError('no pattern keeps %d frames' % kept)


# The rows the value bound is tested on: speech with a noise floor against itself plus noise, and loud / quiet rows of noise
# (every band of every kept frame holds energy).  test_stoi_host.py asserts S.centred_ratios >= 1e-3 on each.
def bound_rows():
    keys = [('speech', 10), ('speech', 0)]
    keys += [pattern_with_kept(k) for k in (30, 31)]
    keys += [pattern_with_kept(SEG_CHUNK + N_SEG - 1 + d, seed=3) for d in (-1, 0, 1)]       # 63, 64 and 65 segments
    keys += [pattern_with_kept(36, lead=5), pattern_with_kept(36, gap_at=17, gap=6), pattern_with_kept(36, trail=5)]
    return keys



def same_results(got, want):
    """two (records, kept_index, envelopes) answers of Engine.stoi: the same bits in everything the stage writes -- the records,
    and of every row the first `kept` indices and envelope columns (what lies behind them is never touched)"""
    if got[0].tobytes() != want[0].tobytes():
        return False
    for b, r in enumerate(got[0]):
        k = int(r['kept'])
        if got[1][b, :k].tobytes() != want[1][b, :k].tobytes() or got[2][b, :, :, :k].tobytes() != want[2][b, :, :, :k].tobytes():
            return False
    return True
