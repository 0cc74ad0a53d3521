"""numpy oracle of tts_dtw (include/sstts_hip.h has the definition): dynamic time warping of two feature sequences under the
Euclidean distance of their frames, in two forms that must agree bit for bit -- ``dtw_sequential`` restates the definition cell
by cell, ``dtw_diagonals`` evaluates a whole anti-diagonal at once (what makes the largest shapes affordable).  Every operation is
an IEEE double operation of its own: numpy neither fuses a product into a sum nor reorders them, and np.sqrt is correctly rounded.

``order`` is the order in which the candidates are taken -- the definition's is ``ORDER`` = diagonal, up, left; any other order
is there to show that the tie rule matters (tests/test_dtw_host.py)."""
import numpy as np

DIAG, UP, LEFT, START = 0, 1, 2, 3
ORDER = (DIAG, UP, LEFT)
STEP = {DIAG: (1, 1), UP: (1, 0), LEFT: (0, 1)}


def local_costs(a, b, D=None):
    """c(i, j) = sqrt(s), s = 0.0; for d < D: t = (double)a[i][d] - (double)b[j][d]; s = s + t * t.  -> (na, nb) float64"""
    a, b = np.asarray(a), np.asarray(b)
    D = a.shape[1] if D is None else D
    s = np.zeros((a.shape[0], b.shape[0]), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for d in range(D):
            t = a[:, d].astype(np.float64)[:, None] - b[:, d].astype(np.float64)[None, :]
            s = s + t * t
        return np.sqrt(s)


def _path(direction, na, nb):
    path = []
    i, j = na - 1, nb - 1
    while True:
        path.append((i, j))
        code = int(direction[i, j])
        if code == START:
            break
        di, dj = STEP[code]
        i, j = i - di, j - dj
    return np.asarray(path[::-1], np.int32).reshape(-1, 2)


def dtw_sequential(a, b, D=None, order=ORDER):
    """-> (cost float64, path_len int, path (path_len, 2) int32), cell by cell as the definition reads"""
    c = local_costs(a, b, D)
    na, nb = c.shape
    Dm = np.zeros((na, nb), np.float64)
    L = np.zeros((na, nb), np.int64)
    direction = np.full((na, nb), START, np.uint8)
    for i in range(na):
        for j in range(nb):
            if i == 0 and j == 0:
                Dm[0, 0], L[0, 0] = c[0, 0], 1
                continue
            best = None
            for code in order:
                di, dj = STEP[code]
                pi, pj = i - di, j - dj
                if pi < 0 or pj < 0:
                    continue
                if best is None or Dm[pi, pj] < Dm[best[1], best[2]]:   # (a comparison with NaN is False)
                    best = (code, pi, pj)
            Dm[i, j] = c[i, j] + Dm[best[1], best[2]]
            L[i, j] = L[best[1], best[2]] + 1
            direction[i, j] = best[0]
    return Dm[-1, -1], int(L[-1, -1]), _path(direction, na, nb)


def diag_range(k, na, nb):
    """first and last row i of anti-diagonal k of an na x nb table (cells (i, k - i))"""
    return max(0, k - (nb - 1)), min(k, na - 1)


def dtw_diagonals(a, b, D=None, order=ORDER):
    """the same results, one anti-diagonal per numpy operation"""
    c = local_costs(a, b, D)
    na, nb = c.shape
    Dm = np.zeros((na, nb), np.float64)
    L = np.zeros((na, nb), np.int64)
    direction = np.full((na, nb), START, np.uint8)
    Dm[0, 0], L[0, 0] = c[0, 0], 1
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(1, na + nb - 1):
            lo, hi = diag_range(k, na, nb)
            i = np.arange(lo, hi + 1)
            j = k - i
            have = np.zeros(i.shape, bool)
            best = np.zeros(i.shape, np.float64)
            best_l = np.zeros(i.shape, np.int64)
            best_c = np.zeros(i.shape, np.uint8)
            for code in order:
                di, dj = STEP[code]
                pi, pj = i - di, j - dj
                exists = (pi >= 0) & (pj >= 0)
                val = Dm[np.maximum(pi, 0), np.maximum(pj, 0)]
                take = exists & (~have | (val < best))
                best = np.where(take, val, best)
                best_l = np.where(take, L[np.maximum(pi, 0), np.maximum(pj, 0)], best_l)
                best_c = np.where(take, np.uint8(code), best_c)
                have |= exists
            Dm[i, j] = c[i, j] + best
            L[i, j] = best_l + 1
            direction[i, j] = best_c
    return Dm[-1, -1], int(L[-1, -1]), _path(direction, na, nb)


def padded_path(path, rows):
    """the (rows, 2) int32 array tts_dtw writes: the path, then (-1, -1)"""
    out = np.full((rows, 2), -1, np.int32)
    out[:len(path)] = path
    return out


def same_bits(x, y):
    """element for element the same float64 bits; a NaN equals a NaN of any sign and payload (no operation here defines them)"""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    if x.shape != y.shape or not np.array_equal(np.isnan(x), np.isnan(y)):
        return False
    ok = ~np.isnan(x)
    return x[ok].tobytes() == y[ok].tobytes()
