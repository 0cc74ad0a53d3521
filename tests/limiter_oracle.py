"""A numpy restatement of the true-peak meter and the look-ahead limiter (include/sstts_hip.h, csrc/limiter_plan.h): every
product, sum and quotient an individually rounded float64 operation in the order the header gives, one utterance at a time.  The
taps come from the library (``_hip.true_peak_filter()``: sin and the Bessel series are its host's), nothing else does.  No GPU."""
import numpy as np

MAX_LOOKAHEAD = 1024
PHASES, TAPS, BEFORE, AFTER = 4, 12, 5, 6
BETA = 4.0
TILE = 2048      # samples a workgroup owns (csrc/limiter_plan.h): what the tests place their tile edges by
FLT_MAX = float(np.finfo(np.float32).max)


def design(beta=BETA):
    """the taps as numpy designs them: what the library's are held against (to a few ulp: another libm, another Bessel series)"""
    h = np.zeros((PHASES, TAPS))
    h[0, BEFORE] = 1.0
    for p in range(1, PHASES):
        d = np.arange(TAPS, dtype=np.float64) - BEFORE - 0.25 * p
        h[p] = np.sinc(d) * np.i0(beta * np.sqrt(1.0 - (d / AFTER) ** 2)) / np.i0(beta)
    return h


def interpolate(x, h):
    """y (n, 4): y[i, p] is the point i + p / 4; column 0 is x itself"""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = len(xd)
    pad = np.zeros(n + BEFORE + AFTER)
    pad[BEFORE:BEFORE + n] = xd
    y = np.empty((n, PHASES))
    y[:, 0] = xd
    with np.errstate(invalid='ignore', over='ignore'):
        for p in range(1, PHASES):
            acc = h[p, 0] * pad[0:n]
            for k in range(1, TAPS):
                acc = acc + h[p, k] * pad[k:k + n]
            y[:, p] = acc
    return y


def envelope(x, h, oversample):
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    finite = np.isfinite(xd)
    a = np.where(finite, np.abs(xd), 0.0)
    if oversample == 4:
        y = interpolate(x, h)
        for p in range(1, PHASES):
            v = np.abs(y[:, p])
            a = np.where(finite & np.isfinite(v) & (v > a), v, a)
    return a


def true_peak(x, h):
    """(true peak, sample peak) of one utterance"""
    return float(np.max(envelope(x, h, 4), initial=0.0)), float(np.max(envelope(x, h, 1), initial=0.0))


def ceiling_float(c):
    """the largest float32 <= c"""
    if c >= FLT_MAX:
        return np.float32(FLT_MAX)
    f = np.float32(c)
    return np.nextafter(f, np.float32(0)) if float(f) > c else f


def gains(x, h, ceiling, lookahead, oversample):
    """(a, r, m, s, g) of one utterance, float64 arrays (n,)"""
    c, L = float(ceiling), int(lookahead)
    a = envelope(x, h, oversample)
    n = len(a)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(a > c, c / a, 1.0)
    idx = np.arange(n)
    m = r.copy()
    for d in range(-L, L + 1):                                   # (exact: any order)
        j = idx + d
        ok = (j >= 0) & (j < n)
        m = np.where(ok, np.minimum(m, r[np.clip(j, 0, n - 1)]), m)
    acc = m[np.clip(idx - L, 0, n - 1)]
    for d in range(-L + 1, L + 1):                               # ascending j = i + d
        acc = acc + m[np.clip(idx + d, 0, n - 1)]
    s = acc / float(2 * L + 1)
    return a, r, m, s, np.minimum(s, r)


def limit(x, h, ceiling, lookahead, oversample):
    """(out float32 (n,), (over, limited, min_gain)) of one utterance"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a, r, _m, _s, g = gains(x, h, ceiling, lookahead, oversample)
    finite = np.isfinite(x)
    touched = finite & (g < 1.0)
    cf = ceiling_float(float(ceiling))
    with np.errstate(invalid='ignore'):
        v = np.abs((g * x.astype(np.float64)).astype(np.float32))
    out = x.copy()
    out[touched] = np.copysign(np.minimum(v, cf), x)[touched]
    stats = (int(np.count_nonzero(a > float(ceiling))), int(np.count_nonzero(touched)), float(np.min(g[touched], initial=1.0)))
    return out, stats

