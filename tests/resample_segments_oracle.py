"""Oracle of the segment-wise resampler (tts_resample_segments): a float64 numpy restatement of the arithmetic include/sstts_hip.h
states, built on tests/resample_oracle.py -- its window, constants and bound -- with its own position arithmetic for a segment's
``first``, plus the plan: the checks of a segment list in the library's order with the library's words, the output samples of
every segment and row, and the cut into launches and tiles.  A segment is a row ``(row, first, samples, ratio)`` (``reserved``
travels as an optional fifth element)."""
import numpy as np

import resample_oracle as R

MAX_SEGMENTS = 4096
SEGMENTS_PER_LAUNCH = 64
MAX_RATIOS = 16
TILE = 256
MAX_N_OUT = 1 << 30


def count(samples, ratio):
    """output samples of a segment: a copy keeps its samples, anything else is resampy's int(samples * ratio)"""
    return int(samples) if ratio == 1.0 else R.resampled_valid(samples, ratio)


def plan(segments, B, n, n_samples=None):
    """``(why, n_out, counts)``: why is None for a legal list, else the refusal in the library's words (n_out and counts are
    then None)"""
    S = len(segments)
    if B < 1 or n < 1 or S < 1:
        return 'need B, n, S >= 1', None, None
    if S > MAX_SEGMENTS:
        return '{} segments are more than tts_resample_segments_max() = {}'.format(S, MAX_SEGMENTS), None, None
    if B > S:
        return '{} rows of {} segments: no row is without a segment'.format(B, S), None, None
    ns = [n] * B if n_samples is None else [int(v) for v in n_samples]
    for b, v in enumerate(ns):
        if not 1 <= v <= n:
            return 'n_samples[{}] = {} is not in 1 .. n = {}'.format(b, v, n), None, None
    rows = [int(q[0]) for q in segments]
    if rows[0] != 0:
        return 'row of segment 0 is {}: the rows start at 0'.format(rows[0]), None, None
    for s in range(1, S):
        if rows[s] - rows[s - 1] not in (0, 1):
            return 'row of segment {} is {} and follows {}: the rows are non-decreasing and none is without a segment'.format(
                s, rows[s], rows[s - 1]), None, None
    if rows[-1] != B - 1:
        return 'row of segment {} is {}: the last row is B - 1 = {}'.format(S - 1, rows[-1], B - 1), None, None
    n_out, counts, below, extra_at = [0] * B, [], [], None
    for s, q in enumerate(segments):
        row, first, samples, ratio = q[:4]
        reserved = q[4] if len(q) > 4 else 0
        if samples < 1:
            return 'segment {} has {} samples: at least 1 is needed'.format(s, samples), None, None
        if first < 0 or first + samples > ns[row]:
            return 'segment {} reads samples {} .. {} of row {}, which has 0 .. {}'.format(s, first, first + samples - 1, row, ns[row] - 1), None, None
        if not R.ratio_ok(ratio):
            return 'segment {} has a ratio that is not finite or lies outside [0.25, 4]'.format(s), None, None
        if reserved != 0:
            return 'segment {} has reserved = {}, which must be 0'.format(s, reserved), None, None
        if ratio < 1.0 and ratio not in below:
            if len(below) < MAX_RATIOS:
                below.append(ratio)
            elif extra_at is None:
                extra_at = s
        counts.append(count(samples, ratio))
        n_out[row] += counts[-1]
    if extra_at is not None:
        return 'segment {} brings distinct ratio below 1 number {}: a call takes tts_resample_segments_max_ratios() = {}'.format(
            extra_at, MAX_RATIOS + 1, MAX_RATIOS), None, None
    return None, n_out, counts


def room(n_out, N_out):
    """the refusal of an N_out behind a legal list, or None"""
    for b, v in enumerate(n_out):
        if v > N_out:
            return 'N_out = {} is below n_out[{}] = {}'.format(N_out, b, v)
    if N_out > MAX_N_OUT:
        return 'N_out = {} is above 2^30 = {}'.format(N_out, MAX_N_OUT)
    return None


def launches(S):
    return -(-S // SEGMENTS_PER_LAUNCH)


def cut(segments, counts, N_out):
    """The tiles of every launch: a list (one per launch) of lists (one per segment) of ``(o, span, tiles)`` -- a segment owns its
    own output samples, a row's last segment everything up to N_out; a segment that owns nothing has no tile"""
    out, o = [], 0
    for s, q in enumerate(segments):
        last = s + 1 == len(segments) or segments[s + 1][0] != q[0]
        span = N_out - o if last else counts[s]
        if s % SEGMENTS_PER_LAUNCH == 0:
            out.append([])
        out[-1].append((o, span, -(-span // TILE)))
        o = 0 if last else o + counts[s]
    return out


def phase(j, first, ratio):
    """(m, (off, eta, taps) of the left wing, (off, eta, taps) of the right wing) for output sample(s) j of a segment that starts
    at ``first``: the position is measured from there, and the wings are not cut (the row's ends cut them: ``segment``)"""
    scale, step, inc = R.consts(ratio)
    j = np.asarray(j, dtype=np.int64)
    tr = j.astype(np.float64) * inc
    t = tr.astype(np.int64)
    frac = scale * (tr - t.astype(np.float64))
    wings = []
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        f = frac * R.NUM_TABLE
        off = f.astype(np.int64)
        eta = f - off.astype(np.float64)
        wings.append((off, eta, (R.NWIN - off) // step))
    return first + t, wings[0], wings[1]


def segment(x, first, c, ratio):
    """One resampled segment of a row x (n_in,) -- the samples that may be read -> ``(y, sabs, lo, hi)``, float64 and int64 of c
    samples: the sum in the library's order, the sum of |weight| |x| behind it, and the first and last sample of the row that the
    output's window covers (inside the row)"""
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    _scale, step, _inc = R.consts(ratio)
    win, delta = R.window(ratio)
    m, left, right = phase(np.arange(c), first, ratio)
    acc, acc_abs = np.zeros(c), np.zeros(c)
    for wing, (off, eta, taps) in enumerate((left, right)):
        for i in range(int(taps.max()) if c else 0):
            src = m - i if wing == 0 else m + 1 + i
            live = (i < taps) & (src >= 0) & (src < n_in)
            idx = np.where(live, off + i * step, 0)
            w = win[idx] + eta * delta[idx]
            xv = x[np.clip(src, 0, n_in - 1)]
            with np.errstate(invalid='ignore'):
                acc = acc + np.where(live, w * xv, 0.0)
                acc_abs = acc_abs + np.where(live, np.abs(w) * np.abs(xv), 0.0)
    lo = np.clip(m - left[2] + 1, 0, n_in)
    hi = np.clip(m + right[2], -1, n_in - 1)
    return acc, acc_abs, lo, hi


COPY, RESAMPLED = 1, 2


def resample_segments(x, segments, n_samples=None, N_out=None):
    """x (B, n) float32 -> a dict: ``y`` (B, N_out) float64 (a copy's value as it is), ``sabs`` (the scale of the bound, 0 where
    nothing is summed), ``kind`` (0: a zero, COPY, RESAMPLED), ``bits`` (uint32: what a copy or a zero holds bit for bit), ``lo`` /
    ``hi`` (the row's samples an output reads, hi < lo: none) and ``n_out``.  N_out None: the longest row, at least 1.  The
    samples at and behind n_samples[b] are not read, whatever they hold."""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    why, n_out, counts = plan(segments, B, n, n_samples)
    assert why is None, why
    N_out = max(max(n_out), 1) if N_out is None else N_out
    assert room(n_out, N_out) is None
    ns = [n] * B if n_samples is None else [int(v) for v in n_samples]
    out = dict(y=np.zeros((B, N_out)), sabs=np.zeros((B, N_out)), kind=np.zeros((B, N_out), np.int8), bits=np.zeros((B, N_out), np.uint32),
               lo=np.zeros((B, N_out), np.int64), hi=np.full((B, N_out), -1, np.int64), n_out=n_out)
    o = [0] * B
    for q, c in zip(segments, counts):
        row, first, _samples, ratio = q[:4]
        at = slice(o[row], o[row] + c)
        if ratio == 1.0:
            out['y'][row, at] = x[row, first:first + c]
            out['bits'][row, at] = x[row, first:first + c].view(np.uint32)
            out['kind'][row, at] = COPY
            out['lo'][row, at] = out['hi'][row, at] = np.arange(first, first + c)
        elif c:
            out['y'][row, at], out['sabs'][row, at], out['lo'][row, at], out['hi'][row, at] = segment(x[row, :ns[row]], first, c, ratio)
            out['kind'][row, at] = RESAMPLED
        o[row] += c
    assert o == n_out
    return out
