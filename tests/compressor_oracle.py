"""The compressor in numpy: csrc/compressor_plan.h restated operation by operation in IEEE double -- the detector's two recurrences,
the cut of a row into segments of 256 samples, the five passes (A, chain A, B, chain B, C) and the gain computer.  It is vectorised
ACROSS segments and loops over the positions inside one, so every product, sum and maximum is a single rounded numpy operation on
arrays; the GPU's envelope is held to it bit for bit, its output to a bound (log10 and pow lie between).  ``plain`` is the
recurrence without a cut, sample by sample.  No GPU, no library."""
import collections
import math

import numpy as np

import equalizer_oracle as EO

SEG, TILE_SEGS, TILE, UTTS = EO.SEG, EO.TILE_SEGS, EO.TILE, EO.UTTS
SR_MIN, SR_MAX = EO.SR_MIN, EO.SR_MAX
THRESHOLD_MIN, THRESHOLD_MAX = -80.0, 0.0
KNEE_MAX = 40.0
MAKEUP_MIN, MAKEUP_MAX = -24.0, 24.0
MS_MAX = 10000.0

Params = collections.namedtuple('Params', 'threshold_db slope knee_db makeup_db attack_coeff release_coeff')
# threshold, ratio, knee, attack ms, release ms, make-up: every preset is untuned
PROFILES = {
    'speech': (-18.0, 3.0, 6.0, 5.0, 100.0, 3.0),
    'telephony': (-20.0, 4.0, 6.0, 3.0, 80.0, 6.0),
    'small-speaker': (-24.0, 6.0, 10.0, 2.0, 60.0, 8.0),
}


# ---- the design
def coefficient(ms, sr):
    return 0.0 if ms == 0 else math.exp(-1.0 / (ms * 1e-3 * sr))


def design(sr, attack_ms, release_ms):
    if not (SR_MIN <= sr <= SR_MAX and 0.0 <= attack_ms <= MS_MAX and 0.0 <= release_ms <= MS_MAX):
        raise ValueError('unsupported')
    return coefficient(attack_ms, sr), coefficient(release_ms, sr)


def params(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db, sr):
    """the parameters of (threshold, ratio, knee, attack ms, release ms, make-up) at a sampling rate; ratio may be inf"""
    aA, aR = design(sr, attack_ms, release_ms)
    return Params(float(threshold_db), 1.0 / ratio, float(knee_db), float(makeup_db), aA, aR)


def profile(name, sr):
    T, R, W, a, r, m = PROFILES[name]
    return params(T, R, W, a, r, m, sr)


def params_refused(p):
    p = Params(*p)
    ok = (THRESHOLD_MIN <= p.threshold_db <= THRESHOLD_MAX and 0.0 <= p.slope <= 1.0 and 0.0 <= p.knee_db <= KNEE_MAX and
          MAKEUP_MIN <= p.makeup_db <= MAKEUP_MAX and 0.0 <= p.attack_coeff < 1.0 and 0.0 <= p.release_coeff < 1.0)
    return not ok


# ---- the cut
segments, segment_len, tiles = EO.segments, EO.segment_len, EO.tiles


def state_doubles(N):
    return 2 * segments(N)


def partials(N):
    return tiles(N)


def power(a):
    """a multiplied out SEG times, one rounded product a time"""
    p = np.float64(1.0)
    for _ in range(SEG):
        p = p * np.float64(a)
    return p


Coef = collections.namedtuple('Coef', 'T s1 W makeup aA bA aR AA AR')


def coef(p):
    p = Params(*p)
    f = np.float64
    return Coef(f(p.threshold_db), f(p.slope) - f(1.0), f(p.knee_db), f(p.makeup_db), f(p.attack_coeff), f(1.0) - f(p.attack_coeff),
                f(p.release_coeff), power(p.attack_coeff), power(p.release_coeff))


# ---- the arithmetic
def detect(k, x, e1, e):
    """one sample into both states, for every lane at once -> (e1, e)"""
    v = np.where(np.isfinite(x), np.abs(x), 0.0)
    e1 = np.maximum(v, k.aR * e1)
    e = k.aA * e + k.bA * e1
    return e1, e


def chain_release(k, c, s):
    return np.maximum(c, k.AR * s)


def chain_attack(k, q, t):
    return k.AA * t + q


def level(env, ulps=0):
    """L = 20 log10(e); ``ulps``: moved by that many units in the last place (what a device's log10 may differ by)"""
    with np.errstate(all='ignore'):
        L = 20.0 * np.log10(env)
    if ulps:
        step = np.spacing(np.abs(L))
        L = np.where(np.isfinite(L), L + ulps * step, L)
    return L


def reduction(k, L, dtype=np.float64):
    """r (<= 0) in dB at the level L, computed directly: -inf gives 0"""
    f = dtype
    L = np.asarray(L, dtype)
    d = L - f(k.T)
    d2 = f(2.0) * d
    W, s1 = f(k.W), f(k.s1)
    with np.errstate(all='ignore'):
        above = s1 * d
        u = d + W / f(2.0)
        knee = s1 * (u * u) / (f(2.0) * W) if W > 0 else above
    return np.where(d2 <= -W, f(0.0), np.where(d2 >= W, above, knee)).astype(dtype)


def apply_gain(k, x, r, dtype=np.float64):
    """-> (y in ``dtype`` before the rounding to float32, identity mask): y = x * 10^((r + makeup) / 20)"""
    f = dtype
    z = np.asarray(r, dtype) + f(k.makeup)
    with np.errstate(all='ignore'):
        g = np.power(f(10.0), z / f(20.0))
        y = np.asarray(x, dtype) * g
    return y, z == 0


Result = collections.namedtuple('Result', 'out y envelope r identity c s q t')


def compress(x, p, ulps=0, gain_dtype=np.float64):
    """the five passes over one row ``x`` (float32)"""
    k = coef(p)
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    n = len(x)
    n_seg = segments(n)
    pad = np.zeros(n_seg * SEG)
    pad[:n] = x
    xs = pad.reshape(n_seg, SEG).T.copy()             # xs[i]: sample i of every segment
    zero = np.zeros(n_seg)
    with np.errstate(all='ignore'):
        e1, e = zero.copy(), zero.copy()
        for i in range(SEG):                          # pass A
            e1, e = detect(k, xs[i], e1, e)
        c = e1                                        # (the last column is never read)
        s = np.zeros(n_seg)
        for g in range(n_seg - 1):                    # chain A
            s[g + 1] = chain_release(k, c[g], s[g])
        e1, e = s.copy(), zero.copy()
        for i in range(SEG):                          # pass B
            e1, e = detect(k, xs[i], e1, e)
        q = e
        t = np.zeros(n_seg)
        for g in range(n_seg - 1):                    # chain B
            t[g + 1] = chain_attack(k, q[g], t[g])
        e1, e = s.copy(), t.copy()
        env = np.empty((SEG, n_seg))
        for i in range(SEG):                          # pass C
            e1, e = detect(k, xs[i], e1, e)
            env[i] = e
    env = env.T.reshape(-1)[:n].copy()
    r = reduction(k, level(env.astype(gain_dtype), ulps), gain_dtype)   # (in float32 the logarithm itself is float32's)
    y, identity = apply_gain(k, x, r, gain_dtype)
    with np.errstate(all='ignore'):
        out = np.where(identity, x32, y.astype(np.float32))
    return Result(out, np.where(identity, x, y.astype(np.float64)), env, r.astype(np.float64), identity, c, s, q, t)


def stats(res):
    """(n, reduced, max_reduction_db, peak_out) of a row's result"""
    finite = np.abs(res.out[~np.isnan(res.out)])
    return (len(res.out), int(np.sum(res.r < 0)), float(np.max(-res.r, initial=0.0)), np.float32(finite.max() if len(finite) else 0.0))


def plain(x, p):
    """the detector over the whole row without a cut, in double: e of every sample"""
    k = coef(p)
    x = np.asarray(x, np.float32).astype(np.float64)
    env = np.empty(len(x))
    e1 = e = np.float64(0.0)
    for i, v in enumerate(x):
        e1, e = detect(k, v, e1, e)
        env[i] = e
    return env


def static_gain_db(p, level_db):
    """the static curve: the gain in dB a steady level meets (make-up included)"""
    k = coef(p)
    return float(reduction(k, np.float64(level_db)) + k.makeup)
