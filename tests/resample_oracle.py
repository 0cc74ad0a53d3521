"""Float64 numpy oracle of the band-limited resampler: resampy 0.2 ``resample_f`` with the 'kaiser_best' filter, which is
librosa 0.6 ``resample(..., res_type='kaiser_best')`` (reference audio/effects.py:9-43, audio/io.py load_wav).  resampy and
librosa are not installed and resampy's filter ships as a data file, so the filter is regenerated from resampy's published design
parameters and the parity is "unpinned": this restatement is the yardstick (include/sstts_hip.h states the same arithmetic).

For ratio rho = target rate / source rate and output sample t of an utterance of n_in samples:
    tr = t * (1 / rho), m = int(tr), frac = scale * (tr - m)               scale = min(1, rho), step = int(scale * 512)
    f = frac * 512, off = int(f), eta = f - off
    y = sum_i (win[off + i step] + eta delta[off + i step]) x[m - i]        i < min(m + 1, (32769 - off) // step)
      + the same with frac = scale - frac on x[m + 1 + k]                   k < min(n_in - m - 1, (32769 - off) // step)
"""
import numpy as np

NUM_ZEROS = 64
NUM_TABLE = 512
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596
HALF = NUM_TABLE * NUM_ZEROS
NWIN = HALF + 1
RATIO_MIN, RATIO_MAX = 0.25, 4.0

_BASE = None


def half_window():
    """kaiser(2 n + 1, beta)[n + j] * rolloff * sinc(rolloff * j / 512), j = 0 .. n = 32768 (float64, 32769 values)"""
    global _BASE
    if _BASE is None:
        j = np.arange(NWIN, dtype=np.float64)
        _BASE = np.kaiser(2 * HALF + 1, BETA)[HALF:] * ROLLOFF * np.sinc(ROLLOFF * j / NUM_TABLE)
        _BASE.setflags(write=False)
    return _BASE


def window(rho):
    """(win, delta) of a ratio: win *= rho below 1; delta[j] = win[j + 1] - win[j], delta[n] = 0"""
    win = half_window().copy()
    if rho < 1.0:
        win *= rho
    delta = np.zeros_like(win)
    delta[:-1] = win[1:] - win[:-1]
    return win, delta


def consts(rho):
    rho = np.float64(rho)
    scale = min(np.float64(1.0), rho)
    return scale, int(scale * NUM_TABLE), np.float64(1.0) / rho


def ratio_ok(rho):
    return bool(RATIO_MIN <= rho <= RATIO_MAX)


def resampled_valid(n, rho):
    return int(np.float64(n) * np.float64(rho)) if n >= 1 else 0


def resampled_length(n, rho):
    return int(np.ceil(np.float64(n) * np.float64(rho))) if n >= 1 else 0


def phase(t, n_in, rho):
    """(m, (off, eta, taps) of the left wing, (off, eta, taps) of the right wing) for output sample(s) t"""
    scale, step, inc = consts(rho)
    t = np.asarray(t, dtype=np.int64)
    tr = t.astype(np.float64) * inc
    m = tr.astype(np.int64)
    frac = scale * (tr - m.astype(np.float64))
    wings = []
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        f = frac * NUM_TABLE
        off = f.astype(np.int64)
        eta = f - off.astype(np.float64)
        room = m + 1 if wing == 0 else n_in - m - 1
        taps = np.minimum(np.maximum(room, 0), (NWIN - off) // step)
        wings.append((off, eta, taps))
    return m, wings[0], wings[1]


def resample(x, rho, n_out=None, reverse=False, table_eps=None, drop_tap=None, eta_zero=False, m_shift=0):
    """One utterance x (n_in,) -> (y, sabs), both float64 of n_out samples (default ceil(n_in * rho)): y holds
    min(int(n_in * rho), n_out) computed samples and zeros behind them, sabs the sum of |weight| |x| behind each of them -- the
    scale of the bound.  The variants are for the bound model only: ``reverse`` sums the taps in the opposite order,
    ``table_eps`` perturbs the table by that much relative (a fixed sign pattern), ``drop_tap`` = (wing, i) leaves one tap
    out, ``eta_zero`` forces the interpolation weight to 0, ``m_shift`` moves m."""
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    scale, step, inc = consts(rho)
    win, delta = window(rho)
    if table_eps:
        sign = np.where(np.arange(NWIN) % 2 == 0, 1.0, -1.0)
        win = win * (1.0 + table_eps * sign)
        delta = np.zeros_like(win)
        delta[:-1] = win[1:] - win[:-1]
    n_valid = resampled_valid(n_in, rho)
    n_out = resampled_length(n_in, rho) if n_out is None else int(n_out)
    keep = min(n_valid, n_out)
    y = np.zeros(n_out)
    sabs = np.zeros(n_out)
    if keep == 0:
        return y, sabs
    m, left, right = phase(np.arange(keep), n_in, rho)
    m = m + m_shift
    terms = []   # (products, |products|) in the order the reference sums them
    for wing, (off, eta, taps) in enumerate((left, right)):
        if eta_zero:
            eta = np.zeros_like(eta)
        if m_shift:
            taps = np.minimum(np.maximum(m + 1 if wing == 0 else n_in - m - 1, 0), (NWIN - off) // step)
        for i in range(int(taps.max()) if taps.size else 0):
            live = i < taps
            if drop_tap == (wing, i):
                continue
            idx = np.where(live, off + i * step, 0)
            src = np.where(live, m - i if wing == 0 else m + 1 + i, 0)
            w = win[idx] + eta * delta[idx]
            xv = x[np.clip(src, 0, n_in - 1)]
            with np.errstate(invalid='ignore'):
                p = np.where(live, w * xv, 0.0)
                a = np.where(live, np.abs(w) * np.abs(xv), 0.0)
            terms.append((p, a))
    acc = np.zeros(keep)
    acc_abs = np.zeros(keep)
    for p, a in (reversed(terms) if reverse else terms):
        acc = acc + p
        acc_abs = acc_abs + a
    y[:keep] = acc
    sabs[:keep] = acc_abs
    return y, sabs


def resample_batch(x, rho, n_samples=None, n_out=None):
    """x (B, n) -> (y (B, N_out), sabs (B, N_out)) as tts_resample lays them out; N_out defaults to ceil(longest * rho)"""
    x = np.asarray(x)
    B, n = x.shape
    ns = [n] * B if n_samples is None else [int(v) for v in n_samples]
    N = resampled_length(max(ns), rho) if n_out is None else int(n_out)
    y = np.zeros((B, N))
    s = np.zeros((B, N))
    for b in range(B):
        y[b], s[b] = resample(x[b, :ns[b]], rho, n_out=N)
    return y, s


def bound(y64, sabs):
    """|y - y64| <= 2^-24 |y64| + 2^-36 sum |w| |x|: one rounding to float32, and the double accumulation of at most 514 taps
    (5.7e-14 of sum |w| |x|) plus libm against numpy in the table (1e-14), both under 2^-36 = 1.5e-11 a hundredfold."""
    with np.errstate(invalid='ignore'):
        return 2.0 ** -24 * np.abs(y64) + 2.0 ** -36 * sabs


def covers(n_in, rho, src):
    """the outputs t (bool array of int(n_in * rho)) whose window reads input sample ``src``"""
    keep = resampled_valid(n_in, rho)
    m, (_o0, _e0, taps_l), (_o1, _e1, taps_r) = phase(np.arange(keep), n_in, rho)
    return ((src <= m) & (src > m - taps_l)) | ((src > m) & (src <= m + taps_r))
