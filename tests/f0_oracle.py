"""The sequential statement of tts_f0 and tts_f0_compare (include/sstts_hip.h) in numpy float64: what csrc/f0.hip is held to bit for
bit.  Vectorised across utterances of one length, frames and lags; j is walked in order, every product and every sum is a
numpy operation of its own (numpy fuses nothing), and the running sum of the normalisation is np.cumsum, which adds in index
order.  :func:`decide_walk` states the decisions of one frame as plain walks, for tests/test_f0_host.py to hold the vectorised
form against."""
import math

import numpy as np


def frames(n, hop):
    return 1 + n // hop


def first_sample(t, hop, W, tau_max):
    return t * hop - (W + tau_max) // 2


def lag_bounds(sr, fmin, fmax):
    return max(2, int(sr // fmax)), int(math.ceil(sr / fmin))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view))


def normalised_difference(x, hop, W, tau_max):
    """x: (R, n) float32, R utterances of n samples -> (q, c_last): q (R, T, tau_max + 1) float64 with q[..., 0] unused (1.0),
    c_last (R, T) the final running sum of every frame."""
    x = np.asarray(x, np.float32)
    R, n = x.shape
    T = frames(n, hop)
    half = (W + tau_max) // 2
    total = half + (T - 1) * hop + W + tau_max
    xx = np.zeros((R, max(total, half + n)), np.float64)    # x(i) = 0.0 outside [0, n)
    xx[:, half:half + n] = x.astype(np.float64)
    at = np.arange(T) * hop                                  # s0 + half
    taus = np.arange(1, tau_max + 1)
    d = np.zeros((R, T, tau_max), np.float64)
    with np.errstate(all='ignore'):
        for j in range(W):
            u = xx[:, at + j][:, :, None] - xx[:, (at + j)[:, None] + taus[None, :]]
            d = d + u * u
        c = np.cumsum(d, axis=-1)                            # c = c + d[tau], tau ascending
        q = np.where(c == 0.0, 1.0, (d * taus.astype(np.float64)) / c)
    return np.concatenate([np.ones((R, T, 1)), q], axis=-1), c[..., -1]


def decide(q, c_last, sr, tau_min, tau_max, threshold):
    """The threshold, the descent and the interpolation of every frame -> (f0, aperiodicity) float32, shaped like c_last."""
    lead = c_last.shape
    q2 = q.reshape(-1, q.shape[-1])
    rng = q2[:, tau_min:tau_max + 1]
    idx = np.arange(tau_min, tau_max + 1)
    with np.errstate(all='ignore'):
        below = rng < threshold
        voiced = below.any(axis=1)
        tau1 = tau_min + np.argmax(below, axis=1)
        best = tau_min + np.argmin(np.where(np.isnan(rng), np.inf, rng), axis=1)    # the first index of the minimum
        nxt = q2[:, tau_min + 1:tau_max + 1]
        stop = np.concatenate([~(nxt < rng[:, :-1]), np.ones((q2.shape[0], 1), bool)], axis=1)
        star = tau_min + np.argmax(stop & (idx[None, :] >= tau1[:, None]), axis=1)
        rows = np.arange(q2.shape[0])
        a, b = q2[rows, star - 1], q2[rows, star]
        g = q2[rows, np.minimum(star + 1, tau_max)]
        den = (a + g) - (b + b)
        ok = (star < tau_max) & (a >= b) & (g >= b) & (den > 0)
        delta = np.where(ok, (0.5 * (a - g)) / np.where(ok, den, 1.0), 0.0)
        f0 = (sr / (star.astype(np.float64) + delta)).astype(np.float32)
        ap = b.astype(np.float32)
        f0 = np.where(voiced, f0, np.float32(0.0))
        ap = np.where(voiced, ap, q2[rows, best].astype(np.float32))
        bad = ~np.isfinite(c_last.reshape(-1))
        f0 = np.where(bad, np.float32(np.nan), f0).astype(np.float32)
        ap = np.where(bad, np.float32(np.nan), ap).astype(np.float32)
    return f0.reshape(lead), ap.reshape(lead)


def decide_walk(q, c_last, sr, tau_min, tau_max, threshold):
    """One frame (q: (tau_max + 1,)), as the header words it -> (f0, aperiodicity) float32"""
    if not np.isfinite(c_last):
        return np.float32(np.nan), np.float32(np.nan)
    tau1 = None
    for tau in range(tau_min, tau_max + 1):
        if q[tau] < threshold:
            tau1 = tau
            break
    if tau1 is None:
        best = tau_min
        for tau in range(tau_min + 1, tau_max + 1):
            if q[tau] < q[best]:
                best = tau
        return np.float32(0.0), np.float32(q[best])
    star = tau1
    while not (star == tau_max or not q[star + 1] < q[star]):
        star += 1
    delta = 0.0
    if star < tau_max:
        a, b, g = q[star - 1], q[star], q[star + 1]
        den = (a + g) - (b + b)
        if a >= b and g >= b and den > 0:
            delta = (0.5 * (a - g)) / den
    with np.errstate(all='ignore'):
        return np.float32(np.float64(sr) / (np.float64(star) + delta)), np.float32(q[star])


def f0(x, sr, hop, W, tau_min, tau_max, threshold, n_samples=None, T=None):
    """tts_f0 on (B, N) float32 rows -> (f0, aperiodicity) float32 (B, T), T = frames(N, hop) unless given.  Rows are cut to
    their own lengths first, so samples at or behind them cannot reach a result."""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    T = frames(N, hop) if T is None else T
    out = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    lens = [N] * B if n_samples is None else [int(n) for n in n_samples]
    for n in sorted(set(lens)):
        rows = [b for b in range(B) if lens[b] == n]
        q, c_last = normalised_difference(x[rows, :n], hop, W, tau_max)
        f, a = decide(q, c_last, sr, tau_min, tau_max, threshold)
        out[0][rows, :f.shape[1]] = f
        out[1][rows, :a.shape[1]] = a
    return out


def compare(f0_a, f0_b, path):
    """tts_f0_compare of one pair: f0_a (Ta,), f0_b (Tb,) float32, path (rows, 2) -> (counts int32 (5,), s_hz, s_cents, sum |z|):
    s_hz is what the kernel must give bit for bit; s_cents is the float64 evaluation with math.log2, and sum |z| scales its bound."""
    counts = np.zeros(5, np.int32)
    s_hz, s_cents, abs_z = np.float64(0.0), np.float64(0.0), np.float64(0.0)
    with np.errstate(all='ignore'):
        for i, j in np.asarray(path).tolist():
            if i < 0 or j < 0:
                continue
            fa, fb = np.float64(f0_a[i]), np.float64(f0_b[j])
            counts[0] += 1
            if np.isnan(fa) or np.isnan(fb):
                counts[4] += 1
            elif (fa > 0) != (fb > 0):
                counts[2] += 1
            elif fa > 0:
                counts[1] += 1
                u = fa - fb
                s_hz = s_hz + u * u
                if abs(u) > 0.2 * fb:
                    counts[3] += 1
                ratio = fa / fb
                z = np.float64(1200.0) * np.float64(math.log2(ratio)) if 0 < ratio < np.inf else np.float64(1200.0) * np.log2(ratio)
                s_cents = s_cents + z * z
                abs_z = abs_z + abs(z)
    return counts, s_hz, s_cents, abs_z


def cents_bound(s64, abs_z):
    """|S - S64| <= 2e-12 sum |z_k| + 1e-15 S64 (include/sstts_hip.h)"""
    return 2e-12 * abs_z + 1e-15 * s64
