"""The equaliser in numpy: csrc/equalizer_plan.h restated operation by operation in IEEE double -- the design of a section and of
the profiles, the cut of a row into segments of 256 samples, the three passes over the segments and the chain between them.  It is
vectorised ACROSS segments and loops over the positions inside one, so every product and sum is a single rounded numpy operation
on arrays; the GPU results are held to it bit for bit.  ``plain`` is the recurrence without a cut, sample by sample, which shares
nothing with the segmented form but the coefficients.  No GPU, no library."""
import numpy as np

MAX_SECTIONS = 8
SEG = 256
TILE_SEGS = 64
TILE = TILE_SEGS * SEG
UTTS = 64
SR_MIN, SR_MAX = 8000, 192000
F_MIN, F_MAX = 1e-4, 0.49
Q_MIN, Q_MAX = 0.1, 30.0
GAIN_MIN, GAIN_MAX = -40.0, 24.0
Q_BUTTER2 = 0.7071067811865476
Q_BUTTER4 = (0.5411961001461969, 1.3065629648763766)
LOWPASS, HIGHPASS, PEAK, LOWSHELF, HIGHSHELF = range(5)
KINDS = {'lowpass': LOWPASS, 'highpass': HIGHPASS, 'peak': PEAK, 'lowshelf': LOWSHELF, 'highshelf': HIGHSHELF}

PROFILES = {
    'telephony': ((HIGHPASS, 300.0, Q_BUTTER4[0], 0.0), (HIGHPASS, 300.0, Q_BUTTER4[1], 0.0),
                  (LOWPASS, 3400.0, Q_BUTTER4[0], 0.0), (LOWPASS, 3400.0, Q_BUTTER4[1], 0.0)),
    'small-speaker': ((HIGHPASS, 150.0, Q_BUTTER4[0], 0.0), (HIGHPASS, 150.0, Q_BUTTER4[1], 0.0), (PEAK, 3000.0, 1.0, 3.0)),
    'rumble': ((HIGHPASS, 20.0, 0.7071, 0.0),),
    'bright': ((HIGHSHELF, 6000.0, Q_BUTTER2, 3.0),),
    'warm': ((HIGHSHELF, 6000.0, Q_BUTTER2, -3.0), (LOWSHELF, 200.0, Q_BUTTER2, 2.0)),
}


# ---- the design
def design(kind, sr, f0, q=Q_BUTTER2, gain_db=0.0):
    """b0 b1 b2 a1 a2 by the formulas of the plan header; ValueError outside the limits"""
    if kind not in range(5):
        raise ValueError('kind')
    if not (SR_MIN <= sr <= SR_MAX and F_MIN * sr <= f0 <= F_MAX * sr and Q_MIN <= q <= Q_MAX):
        raise ValueError('unsupported')
    if kind >= PEAK and not GAIN_MIN <= gain_db <= GAIN_MAX:
        raise ValueError('unsupported')
    K = np.tan(np.float64(np.pi) * np.float64(f0) / np.float64(sr))
    KK, KQ = K * K, K / np.float64(q)
    if kind in (LOWPASS, HIGHPASS):
        a0, a1, a2 = 1.0 + KQ + KK, 2.0 * (KK - 1.0), 1.0 - KQ + KK
        b0, b1 = (KK, 2.0 * KK) if kind == LOWPASS else (np.float64(1.0), np.float64(-2.0))
        b2 = b0
    elif kind == PEAK:
        A = np.float64(10.0) ** (np.float64(gain_db) / 40.0)
        b0, b1, b2 = 1.0 + KQ * A + KK, 2.0 * (KK - 1.0), 1.0 - KQ * A + KK
        a0, a1, a2 = 1.0 + KQ / A + KK, b1, 1.0 - KQ / A + KK
    else:
        A = np.float64(10.0) ** (np.float64(gain_db) / 40.0)
        g = np.sqrt(A) * KQ
        p, u, pm, um = 1.0 + A * KK, A + KK, 2.0 * (A * KK - 1.0), 2.0 * (KK - A)
        if kind == LOWSHELF:
            b0, b1, b2, a0, a1, a2 = A * (p + g), A * pm, A * (p - g), u + g, um, u - g
        else:
            b0, b1, b2, a0, a1, a2 = A * (u + g), A * um, A * (u - g), p + g, pm, p - g
    return np.array([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0], np.float64)


def profile(name, sr):
    return np.stack([design(k, sr, f0, q, g) for k, f0, q, g in PROFILES[name]])


def profile_fits(name, sr):
    return all(F_MIN * sr <= f0 <= F_MAX * sr for _k, f0, _q, _g in PROFILES[name])


def response(sos, f, sr):
    """|H| of the cascade at the frequencies f (Hz)"""
    z = np.exp(-2j * np.pi * np.asarray(f, np.float64) / sr)
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in np.asarray(sos, np.float64).reshape(-1, 5):
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return np.abs(h)


# ---- the cut
def segments(n):
    return -(-n // SEG)


def segment_len(n, i):
    return min(SEG, n - i * SEG)


def tiles(n):
    return -(-n // TILE)


def state_doubles(N, S):
    return segments(N) * 2 * S


def transition_doubles(S):
    return (2 * S) ** 2


def lds_bytes():
    return TILE_SEGS * (SEG + 1) * 4


# ---- the arithmetic
def _run(k, st, x):
    """one sample through the cascade for every lane at once; k (S, 5), st: 2 S arrays, updated in place; returns y"""
    for s in range(len(k)):
        c = k[s]
        y = c[0] * x + st[2 * s]
        st[2 * s] = (c[1] * x - c[3] * y) + st[2 * s + 1]
        st[2 * s + 1] = c[2] * x - c[4] * y
        x = y
    return x


def _k(sos):
    k = np.asarray(sos, np.float64).reshape(-1, 5)
    assert 1 <= len(k) <= MAX_SECTIONS
    return k


def transition(sos):
    """(2 S, 2 S): column j is the state the recurrence ends in from the unit state j on SEG samples of zero input"""
    k = _k(sos)
    D = 2 * len(k)
    st = [np.eye(D)[r].copy() for r in range(D)]      # st[r][j]: value r of the run that started from unit state j
    zero = np.zeros(D)
    for _ in range(SEG):
        _run(k, st, zero)
    return np.stack(st)


def chain(M, e, S):
    """one link: M S + e, the products summed in ascending column order, e last"""
    a = M[:, 0] * S[0]
    for j in range(1, len(S)):
        a = a + M[:, j] * S[j]
    return a + e


def end_state(sos, x):
    """the state the cascade ends in from the zero state over the samples x (float32), (2 S,)"""
    k = _k(sos)
    st = [np.float64(0.0) for _ in range(2 * len(k))]
    with np.errstate(all='ignore'):
        for v in np.asarray(x, np.float32).astype(np.float64):
            _run(k, st, v)
    return np.array(st)


def equalize64(x, sos):
    """the three passes over one row ``x`` (float32): y in double, before the rounding to float32"""
    k = _k(sos)
    D = 2 * len(k)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = len(x)
    n_seg = segments(n)
    pad =np.zeros(n_seg * SEG)
    pad[:n] = x
    xs = pad.reshape(n_seg, SEG).T.copy()             # xs[i]: sample i of every segment
    with np.errstate(all='ignore'):
        st = [np.zeros(n_seg) for _ in range(D)]
        for i in range(SEG):
            _run(k, st, xs[i])
        e = np.stack(st)                              # (D, n_seg); the last column is never read
        M = transition(k)
        S = np.zeros((D, n_seg))
        cur = np.zeros(D)
        for g in range(n_seg):
            S[:, g] = cur
            if g + 1 < n_seg:
                cur = chain(M, e[:, g], cur)
        st = [S[r].copy() for r in range(D)]
        ys = np.empty((SEG, n_seg))
        for i in range(SEG):
            ys[i] = _run(k, st, xs[i])
    return ys.T.reshape(-1)[:n].copy()


def equalize(x, sos):
    """... and rounded to float32 once: what tts_equalize writes"""
    with np.errstate(all='ignore'):
        return equalize64(x, sos).astype(np.float32)


def plain(x, sos):
    """the recurrence over the whole row without a cut, in double"""
    k = _k(sos)
    st = [np.float64(0.0) for _ in range(2 * len(k))]
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.empty(len(x))
    with np.errstate(all='ignore'):
        for i, v in enumerate(x):
            y[i] = _run(k, st, v)
    return y


def sosfilt_form(sos):
    """the sections as scipy.signal.sosfilt takes them, (S, 6)"""
    k = _k(sos)
    return np.concatenate([k[:, :3], np.ones((len(k), 1)), k[:, 3:]], axis=1)


# ---- the argument checks: 0 legal, 1 TTS_ERR_INVALID
def sections_refused(sos, n_sections):
    if not 1 <= n_sections <= MAX_SECTIONS:
        return True
    k = np.asarray(sos, np.float64).reshape(-1)[:5 * n_sections].reshape(n_sections, 5)
    if not np.all(np.isfinite(k)):
        return True
    return not all(abs(a2) < 1.0 and abs(a1) < 1.0 + a2 for a1, a2 in k[:, 3:])
