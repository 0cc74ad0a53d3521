"""Loudness after ITU-R BS.1770-4 / EBU R 128 in numpy, two ways.

``mean_square`` is the library's arithmetic restated operation by operation in IEEE double (include/sstts_hip.h, tts_loudness, and
csrc/loudness_plan.h): the cut of an utterance into steps, segments and blocks, the three passes over the segments, the block
means and the two gates.  It is vectorised ACROSS segments and loops over the positions inside one, so every product, sum and
quotient is a single rounded numpy operation on arrays; the GPU results are held to it bit for bit.

``plain_mean_square`` is the standard written down directly: scipy's ``sosfilt`` over the whole signal, 400 ms blocks every 100 ms
and the gates.  It shares nothing with the segmented form but the filter coefficients, and the two are held together within
1e-9."""
import numpy as np

SR_MIN, SR_MAX = 8000, 192000
SEGS = 8
Z_ABS = 1.1724653045822981e-07     # the double nearest 10 ** ((-70 + 0.691) / 10)
REL = 0.1

# BS.1770-4 tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def design(sr):
    """the ten coefficients by the formulas of the issue, in Python floats"""
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + high, np.float64)


# ---- the cut
def step(sr):
    return sr // 10


def segment(sr):
    return -(-step(sr) // SEGS)


def segment_lengths(sr):
    c = segment(sr)
    return [c] * (SEGS - 1) + [step(sr) - (SEGS - 1) * c]


def steps(n, sr):
    return n // step(sr)


def blocks(n, sr):
    return max(0, steps(n, sr) - 3)


def lufs(z):
    with np.errstate(divide='ignore', invalid='ignore'):
        return -0.691 + 10.0 * np.log10(np.asarray(z, np.float64))


# ---- the segmented arithmetic
def _run(k, st, x):
    """one sample through the cascade for every segment at once; st: four arrays, updated in place; returns y"""
    y1 = k[0] * x + st[0]
    st[0] = (k[1] * x - k[3] * y1) + st[1]
    st[1] = k[2] * x - k[4] * y1
    y = k[5] * y1 + st[2]
    st[2] = (k[6] * y1 - k[8] * y) + st[3]
    st[3] = k[7] * y1 - k[9] * y
    return y


def transition(k, length):
    """(4, 4): column j is the state the recurrence ends in from the unit state j on zero input"""
    st = [np.eye(4)[r].copy() for r in range(4)]      # st[r][j]: value r of the run that started from unit state j
    zero = np.zeros(4)
    for _ in range(length):
        _run(k, st, zero)
    return np.stack(st)


def mean_square(x, sr, coeffs):
    """-> (z, blocks, blocks that passed both gates) of one utterance ``x`` (float32), with the library's ``coeffs``"""
    k = [np.float64(v) for v in coeffs]
    x = np.asarray(x, np.float32).astype(np.float64)
    s, c = step(sr), segment(sr)
    K = steps(len(x), sr)
    J = K - 3
    if J < 1:
        return 0.0, 0, 0
    lens = np.array(segment_lengths(sr) * K)
    starts = (np.arange(K)[:, None] * s + np.arange(SEGS)[None, :] * c).reshape(-1)
    n_seg = K * SEGS
    xs = np.zeros((c, n_seg))
    for i in range(c):
        live = lens > i
        xs[i, live] = x[starts[live] + i]
    with np.errstate(all='ignore'):
        # pass 1: from the zero state
        st = [np.zeros(n_seg) for _ in range(4)]
        for i in range(c):
            live = lens > i
            new = [a.copy() for a in st]
            _run(k, new, xs[i])
            for r in range(4):
                st[r] = np.where(live, new[r], st[r])
        e = np.stack(st)                                # (4, n_seg)
        # pass 2: the chain
        Mc, Ml = transition(k, c), transition(k, s - (SEGS - 1) * c)
        S = np.zeros((4, n_seg))
        cur = np.zeros(4)
        for g in range(n_seg):
            S[:, g] = cur
            M = Ml if g % SEGS == SEGS - 1 else Mc
            cur = (((M[:, 0] * cur[0] + M[:, 1] * cur[1]) + M[:, 2] * cur[2]) + M[:, 3] * cur[3]) + e[:, g]
        # pass 3: from the true states, the sums of y * y in sample order
        st = [S[r].copy() for r in range(4)]
        acc = np.zeros(n_seg)
        for i in range(c):
            live = lens > i
            new = [a.copy() for a in st]
            y = _run(k, new, xs[i])
            for r in range(4):
                st[r] = np.where(live, new[r], st[r])
            acc = np.where(live, acc + y * y, acc)
        q = acc.reshape(K, SEGS)
        u = q[:, 0] + q[:, 1]
        for i in range(2, SEGS):
            u = u + q[:, i]
        z = (((u[0:J] + u[1:J + 1]) + u[2:J + 2]) + u[3:J + 3]) / np.float64(4 * s)
    return gate(z)


def gate(z):
    """-> (mean square, blocks, blocks that passed) of the block means ``z``, summed in block order"""
    J = len(z)
    if not np.all(np.isfinite(z)):
        return float('nan'), J, 0
    threshold = Z_ABS
    result, passed = 0.0, 0
    for walk in range(2):
        total, count = np.float64(0.0), 0
        for v in z:
            if v > Z_ABS and v > threshold:
                total = total + v
                count += 1
        if not count:
            break
        mean = total / np.float64(count)
        if walk == 0:
            threshold = np.float64(REL) * mean
        else:
            result, passed = float(mean), count
    return result, J, passed


def gain(z, peak, target_lufs, max_peak):
    """the normaliser's gain in Python floats (the library's differs by the roundings of pow alone)"""
    if not (np.isfinite(z) and z > 0.0 and peak > 0.0):
        return 1.0
    g = np.sqrt(np.float64(10.0) ** ((np.float64(target_lufs) + 0.691) / 10.0) / np.float64(z))
    return float(min(g, np.float64(max_peak) / np.float64(peak)))


def finite_peak(x):
    x = np.asarray(x, np.float32)
    a = np.abs(x[np.isfinite(x)])
    return float(a.max()) if a.size else 0.0


# ---- the plain restatement
def plain_block_means(x, sr, coeffs):
    from scipy.signal import sosfilt
    x = np.asarray(x, np.float32).astype(np.float64)
    k = np.asarray(coeffs, np.float64)
    sos = np.array([[k[0], k[1], k[2], 1.0, k[3], k[4]], [k[5], k[6], k[7], 1.0, k[8], k[9]]])
    y = sosfilt(sos, x)
    s = step(sr)
    J = blocks(len(x), sr)
    return np.array([np.mean(y[j * s:j * s + 4 * s] ** 2) for j in range(J)])


def plain_mean_square(x, sr, coeffs, gated=True):
    z = plain_block_means(x, sr, coeffs)
    if not len(z):
        return 0.0
    if not np.all(np.isfinite(z)):
        return float('nan')
    if not gated:
        return float(np.mean(z))
    z = z[z > Z_ABS]
    if not len(z):
        return 0.0
    z = z[z > REL * np.mean(z)]
    return float(np.mean(z)) if len(z) else 0.0
