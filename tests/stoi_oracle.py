"""A numpy float64 restatement of tts_stoi (include/sstts_hip.h, steps 1 to 9): STOI (Taal et al. 2011) and ESTOI (Jensen and
Taal 2016) of a row at 10 kHz.  The window and the band table are the library's (tts_stoi_window, tts_stoi_bands: host
functions, no GPU); the frame energies take the header's summation order, so the kept frames are exact; the transform is
np.fft.rfft -- or, with ``precise``, a direct DFT in np.longdouble -- so envelopes and value are held to ``envelope_bound`` and
``value_bound``, which DESIGN.md derives.  From given envelopes, ``from_envelopes`` is the kernel's arithmetic operation by
operation: its `degenerate` and value are the kernel's bits.

pystoi is not installed, so nothing here is compared with it; the deviations from it (the count of the last frame, the
threshold in the energy domain, no epsilon terms) are listed in DESIGN.md."""
import ctypes
import functools

import numpy as np

from conftest import pkg

W, H, NFFT, J, N = 256, 128, 512, 15, 30
CLIP = 1.0 + 5.623413251903491          # 1 + 10 ** (15 / 20)
RANGE = 1e-4                            # 40 dB in energy
U = 2.0 ** -53
# a radix-2 transform of 512 points loses at most 9 (mu + gamma_4 (sqrt 2 + mu)) <= 9 * 7.7 u of ||Z||_2 (Higham,
# Accuracy and Stability, theorem 24.2, twiddles good to mu = 2 u) -- 8 stages of 256 complex points and the unfolding of the
# real transform are 9 such stages -- and the halving sums of the unfolding 2 u more
C_FFT = 9 * 7.7 + 2.0
C_BAND = 25.0                           # the squares, a band's sum of up to 45 terms and the root: ((45 + 3) / 2 + 1) u of X


@functools.lru_cache(maxsize=None)
def tables():
    """(w float64 (256,), bands int32 (15, 2)) from the library's host functions"""
    lib = pkg('').load_library()
    w = np.zeros(W, np.float64)
    e = np.zeros((J, 2), np.int32)
    assert lib.tts_stoi_window(w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    assert lib.tts_stoi_bands(e.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    w.setflags(write=False)
    e.setflags(write=False)
    return w, e


def frames(n):
    return 0 if n < W else (n - W) // H + 1


def segments(kept):
    return kept - (N - 1) if kept >= N else 0


def energies(x):
    """step 2: E = E + t * t, t = w[i] * x[128 m + i], in ascending i"""
    w, _ = tables()
    x = np.asarray(x, np.float32).astype(np.float64)
    F = frames(len(x))
    E = np.zeros(F)
    at = H * np.arange(F)
    with np.errstate(all='ignore'):
        for i in range(W):
            t = w[i] * x[at + i]
            E = E + t * t
    return E


def kept_frames(E):
    """step 3: the indices of the kept frames, ascending"""
    ok = E[~np.isnan(E)]
    emax = ok.max() if ok.size else 0.0
    with np.errstate(all='ignore'):
        return np.nonzero(E > emax * RANGE)[0].astype(np.int32)


def compact(x, idx):
    """step 4: the overlap-add of the kept frames' windowed samples, in ascending frame order"""
    w, _ = tables()
    x = np.asarray(x, np.float32).astype(np.float64)
    out = np.zeros((len(idx) - 1) * H + W if len(idx) else 0)
    with np.errstate(all='ignore'):
        for k, m in enumerate(idx):
            out[H * k:H * k + W] = out[H * k:H * k + W] + w * x[H * m:H * m + W]
    return out


def windowed(xs, kept):
    """z[m][i] = w[i] * xs[128 m + i]"""
    w, _ = tables()
    at = H * np.arange(kept)[:, None] + np.arange(W)[None, :]
    with np.errstate(all='ignore'):
        return w[None, :] * xs[at] if kept else np.zeros((0, W))


@functools.lru_cache(maxsize=None)
def _dft_longdouble(lo, hi):
    pi = 4 * np.arctan(np.longdouble(1))
    k = np.arange(lo, hi)[:, None] * np.arange(W)[None, :] % NFFT
    ang = 2 * pi * k.astype(np.longdouble) / np.longdouble(NFFT)
    return np.cos(ang), -np.sin(ang)


def envelopes(z, precise=False):
    """step 5: X[j][m] from the windowed frames z (kept, 256)"""
    _, bands = tables()
    out = np.zeros((J, z.shape[0]))
    with np.errstate(all='ignore'):
        if precise:
            zl = z.astype(np.longdouble)
            for j, (lo, hi) in enumerate(bands):
                c, s = _dft_longdouble(int(lo), int(hi))
                re, im = zl @ c.T, zl @ s.T
                out[j] = np.sqrt((re * re + im * im).sum(axis=1)).astype(np.float64)
            return out
        spec = np.fft.rfft(z, NFFT, axis=1)
        P = spec.real ** 2 + spec.imag ** 2
        for j, (lo, hi) in enumerate(bands):
            out[j] = np.sqrt(P[:, lo:hi].sum(axis=1))
    return out


def _minimum(a, b):
    return np.minimum(a, b)   # (a NaN on either side is a NaN)


def _blocks(X):
    """(J, kept) -> (segments, J, N): segment s holds the frames s .. s + 29"""
    S = segments(X.shape[1])
    return np.stack([X[:, s:s + N] for s in range(S)]) if S else np.zeros((0, J, N))


def _seq_sum(v, axis):
    """the sum along ``axis`` from 0.0, one term at a time"""
    v = np.moveaxis(v, axis, 0)
    acc = np.zeros(v.shape[1:])
    for t in range(v.shape[0]):
        acc = acc + v[t]
    return acc


def _unit(v, axis):
    """``v`` minus its mean along ``axis``, over its centred norm; zeros (and a count) where that is 0 -- the kernel's operations"""
    n = v.shape[axis]
    d = v - np.expand_dims(_seq_sum(v, axis) / float(n), axis)
    c = _seq_sum(d * d, axis)
    zero = c == 0.0
    out = np.where(np.expand_dims(zero, axis), 0.0, d / np.expand_dims(np.sqrt(c), axis))
    return out, zero


def from_envelopes(X, Y, extended):
    """steps 6 to 9 from envelopes (J, kept): (value, degenerate, the segments' sums)"""
    S = segments(X.shape[1])
    if S == 0:
        return float('nan'), 0, np.zeros(0)
    with np.errstate(all='ignore'):
        x, y = _blocks(X), _blocks(Y)           # (S, J, N)
        if not extended:
            ny = np.sqrt(_seq_sum(y * y, 2))
            a = np.sqrt(_seq_sum(x * x, 2)) / ny
            yc = _minimum(a[..., None] * y, CLIP * x)
            dx = x - (_seq_sum(x, 2) / float(N))[..., None]
            dy = yc - (_seq_sum(yc, 2) / float(N))[..., None]
            cxy, cxx, cyy = _seq_sum(dx * dy, 2), _seq_sum(dx * dx, 2), _seq_sum(dy * dy, 2)
            bad = (ny == 0.0) | (cxx == 0.0) | (cyy == 0.0)
            r = np.where(bad, 0.0, cxy / (np.sqrt(cxx) * np.sqrt(cyy)))
            sums = _seq_sum(r, 1)
            degenerate = int(bad.sum())
            total = _seq_sum(sums, 0)
            return float(total / float(J * S)), degenerate, sums
        xr, zx = _unit(x, 2)
        yr, zy = _unit(y, 2)
        # the kernel nulls a row by its norm: a row of centred norm 0 is zeros
        xn, cx = _unit(xr, 1)
        yn, cy = _unit(yr, 1)
        prod = xn * yn                           # (S, J, N): summed over the columns t, then the bands j within a column
        sums = np.zeros(S)
        for t in range(N):
            for j in range(J):
                sums = sums + prod[:, j, t]
        sums = sums / float(N)
        degenerate = int(zx.sum() + zy.sum() + cx.sum() + cy.sum())
        return float(_seq_sum(sums, 0) / float(S)), degenerate, sums


def stoi(ref, deg, extended=False, precise=False, round_envelopes=None):
    """One row: a dict of frames, kept, segments, degenerate, value, index (kept,), X and Y (15, kept) and the windowed frames
    zx, zy.  ``round_envelopes``: a dtype the envelopes are rounded to on the way (what a float32 pipeline would hold)."""
    ref, deg = np.asarray(ref, np.float32), np.asarray(deg, np.float32)
    assert ref.shape == deg.shape and ref.ndim == 1
    idx = kept_frames(energies(ref))
    zx, zy = windowed(compact(ref, idx), len(idx)), windowed(compact(deg, idx), len(idx))
    X, Y = envelopes(zx, precise), envelopes(zy, precise)
    if round_envelopes is not None:
        X, Y = X.astype(round_envelopes).astype(np.float64), Y.astype(round_envelopes).astype(np.float64)
    value, degenerate, _ = from_envelopes(X, Y, extended)
    return dict(frames=frames(len(ref)), kept=len(idx), segments=segments(len(idx)), degenerate=degenerate, value=value, index=idx, X=X,
                Y=Y, zx=zx, zy=zy)


# ---- the bounds (DESIGN.md has the derivation)
def envelope_bound(o):
    """(bx, by), each (15, kept): how far a computed X[j][m], Y[j][m] may lie from another computed one.  A transform errs by at
    most C_FFT u sqrt(512) ||z||_2 in the 2-norm of ANY set of bins (each signal has its own), the band sums and roots by
    C_BAND u of the envelope; twice that between two computations."""
    out = []
    for z, env in ((o['zx'], o['X']), (o['zy'], o['Y'])):
        fft = C_FFT * U * np.sqrt(float(NFFT)) * np.sqrt((z ** 2).sum(axis=1))
        out.append(2.0 * (fft[None, :] + C_BAND * U * env))
    return tuple(out)


def _norm(v, axis):
    return np.sqrt((v * v).sum(axis=axis))


def _unit_bound(v, e, axis):
    """elementwise bound of _unit(v) for |dv| <= e elementwise: the centred values move by e + mean(e), the unit vector by that
    over the centred norm plus its own size times the relative change of the norm; (1 + 2 rho) covers the second order"""
    n = v.shape[axis]
    d = v - v.mean(axis=axis, keepdims=True)
    ed = e + e.mean(axis=axis, keepdims=True)
    nd = np.expand_dims(_norm(d, axis), axis)
    rho = np.expand_dims(_norm(ed, axis), axis) / nd
    return (ed / nd + np.abs(d / nd) * rho) * (1.0 + 2.0 * rho) + 4.0 * n * U


def centred_ratios(o, extended):
    """the smallest centred norm over norm among everything the value divides by: the rows of every segment's blocks, and in the
    extended form the columns of the row-normalised blocks too (their norm: a column of 15 unit-row entries)"""
    x, y = _blocks(o['X']), _blocks(o['Y'])
    with np.errstate(all='ignore'):
        if not extended:
            a = _norm(x, 2) / _norm(y, 2)
            yc = np.minimum(a[..., None] * y, CLIP * x)
            rows = [x, yc]
        else:
            rows = [x, y]
        least = min(float((_norm(v - v.mean(axis=2, keepdims=True), 2) / _norm(v, 2)).min()) for v in rows)
        if extended:
            for v in rows:
                r = _unit(v, 2)[0]
                least = min(least, float((_norm(r - r.mean(axis=1, keepdims=True), 1) / _norm(r, 1)).min()))
    return least


def value_bound(o, extended):
    """how far a computed value may lie from another computed one, from the envelope bounds by first-order propagation with the
    second order covered: the correlation of two vectors moves by at most twice the sum of their relative changes"""
    bx, by = envelope_bound(o)
    x, y, ex, ey = _blocks(o['X']), _blocks(o['Y']), _blocks(bx), _blocks(by)
    if x.shape[0] == 0:
        return 0.0
    if not extended:
        Ex, Ey = _norm(ex, 2), _norm(ey, 2)
        a = _norm(x, 2) / _norm(y, 2)
        yc = np.minimum(a[..., None] * y, CLIP * x)
        Eyc = (1.0 + CLIP) * Ex + 2.0 * a * Ey
        rx = Ex / _norm(x - x.mean(axis=2, keepdims=True), 2)
        ry = Eyc / _norm(yc - yc.mean(axis=2, keepdims=True), 2)
        rho = rx + ry
        return float((2.0 * rho + 4.0 * rho * rho + 200.0 * U).mean())
    xr, yr = _unit(x, 2)[0], _unit(y, 2)[0]
    exr, eyr = _unit_bound(x, ex, 2), _unit_bound(y, ey, 2)
    xn, yn = _unit(xr, 1)[0], _unit(yr, 1)[0]
    exn, eyn = _unit_bound(xr, exr, 1), _unit_bound(yr, eyr, 1)
    d = (exn * np.abs(yn) + np.abs(xn) * eyn + exn * eyn).sum(axis=(1, 2)) / float(N)
    return float(d.mean() + 500.0 * U)
