"""float64 numpy oracle of tts_mfcc and of the mel-cepstral distortion built on it (include/sstts_hip.h, audio/metrics.py).
calculate_mfccs (reference audio/features.py:89-113) is librosa.feature.mfcc(S=mel_spec, n_mfcc=n): with S given, the orthonormal
DCT-II of S along the mel axis, first n rows."""
import numpy as np

import dtw_oracle as W


def dct_matrix(n_mels, n_mfcc=None):
    """d[k][n] = sqrt(2 / n_mels) cos(pi k (2 n + 1) / (2 n_mels)), row 0 times 1 / sqrt(2): (n_mfcc, n_mels) float64"""
    n_mfcc = n_mels if n_mfcc is None else n_mfcc
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    n = np.arange(n_mels, dtype=np.float64)[None, :]
    d = np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * n_mels))
    d[0] *= 1.0 / np.sqrt(2.0)
    return d


def mfcc(rows, n_mfcc, n_frames=None, clip01=False, d=None):
    """rows (B, T, n_mels) -> (y, scale), both (B, T, n_mfcc) float64: y = sum_n d[k][n] x[n] with np.dot and scale =
    sum_n |d[k][n]| |x[n]| (what the rounding bound of the kernel is stated in); rows at or behind n_frames[b] give 0."""
    x = np.asarray(rows).astype(np.float64)
    if clip01:
        x = np.clip(x, 0.0, 1.0)
    B, T, n_mels = x.shape
    d = dct_matrix(n_mels, n_mfcc) if d is None else d
    live = np.ones((B, T), bool) if n_frames is None else np.arange(T)[None, :] < np.asarray(n_frames)[:, None]
    y = np.zeros((B, T, n_mfcc))
    scale = np.zeros((B, T, n_mfcc))
    with np.errstate(invalid='ignore'):
        y[live] = np.dot(x[live], d.T)
        scale[live] = np.dot(np.abs(x[live]), np.abs(d).T)
    return y, scale


def bound(y, scale):
    """|out - y| <= 2^-24 |y| + 2^-40 sum_n |d[k][n]| |x[n]|: one rounding to float32, and at most 1026 double roundings plus an
    ulp of cos per term (1027 * 2^-53 < 2^-42) with a factor 4 to spare"""
    return 2.0 ** -24 * np.abs(y) + 2.0 ** -40 * scale


def within_bound(out, y, scale):
    """element by element; a NaN of the oracle must be a NaN of the kernel and nothing else may be one"""
    out = np.asarray(out, np.float64)
    nan = np.isnan(y)
    if not np.array_equal(np.isnan(out), nan):
        return False
    ok = ~nan
    return bool(np.all(np.abs(out[ok] - y[ok]) <= bound(y[ok], scale[ok])))


def mcd_scale(ref_db, max_db):
    """(sqrt(2) / 2) (|ref_db| + |max_db|): dB cepstra of normalised-dB rows -> mel-cepstral distortion in dB"""
    return np.sqrt(2.0) / 2.0 * (abs(float(ref_db)) + abs(float(max_db)))


def mel_cepstral_distortion(mel_a, mel_b, n_a, n_b, n_coeffs, ref_db, max_db, coeffs=None):
    """Per utterance: the float32 cepstra 1 .. n_coeffs of the clipped rows (``coeffs``: the pair of (B, T, n_coeffs + 1) float32
    arrays the device computed, else the oracle's own rounded to float32), aligned by the DTW oracle.
    -> (mcd (B,) float64, cost (B,), path_len (B,), paths list)"""
    if coeffs is None:
        coeffs = tuple(mfcc(m, n_coeffs + 1, n, clip01=True)[0].astype(np.float32) for m, n in ((mel_a, n_a), (mel_b, n_b)))
    ca, cb = coeffs
    B = ca.shape[0]
    cost, plen, paths = np.zeros(B), np.zeros(B, np.int64), []
    for b in range(B):
        na = ca.shape[1] if n_a is None else int(n_a[b])
        nb = cb.shape[1] if n_b is None else int(n_b[b])
        c, l, p = W.dtw_diagonals(ca[b, :na, 1:], cb[b, :nb, 1:], n_coeffs)
        cost[b], plen[b] = c, l
        paths.append(p)
    return mcd_scale(ref_db, max_db) * cost / plen, cost, plen, paths
