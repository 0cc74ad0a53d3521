"""Oracle of the prosody warp (tts_warp_magnitudes): a from-scratch numpy restatement, in float64 and operation by operation, of
the arithmetic include/sstts_hip.h states, plus the plan -- the checks of a segment list in the library's order with the library's
words, the output frames of every segment and row, and the cut into launches and tiles.  A segment is a row
``(row, first, frames, pause, step, gain)``."""
import numpy as np

STEP_MIN, STEP_MAX = 16384, 262144
GAIN_MAX = 16.0
MAX_SEGMENTS = 4096
SEGMENTS_PER_LAUNCH = 64
TILE = 64
MAX_T_OUT = 1 << 30


def count(frames, step):
    """output frames of a speech segment: the j >= 0 with j * step < frames * 65536, in exact integers"""
    c = (frames * 65536) // step
    return c if c * step == frames * 65536 else c + 1


def plan(segments, B, T, n_frames=None):
    """``(why, n_out, counts)``: why is None for a legal list, else the refusal in the library's words (n_out and counts are
    then None)"""
    S = len(segments)
    if B < 1 or T < 1 or S < 1:
        return 'need B, T, S >= 1', None, None
    if S > MAX_SEGMENTS:
        return '{} segments are more than tts_warp_max_segments() = {}'.format(S, MAX_SEGMENTS), None, None
    if B > S:
        return '{} rows of {} segments: no row is without a segment'.format(B, S), None, None
    nf = [T] * B if n_frames is None else [int(v) for v in n_frames]
    for b, n in enumerate(nf):
        if not 1 <= n <= T:
            return 'n_frames[{}] = {} is not in 1 .. T = {}'.format(b, n, T), None, None
    rows = [int(q[0]) for q in segments]
    if rows[0] != 0:
        return 'row of segment 0 is {}: the rows start at 0'.format(rows[0]), None, None
    for s in range(1, S):
        if rows[s] - rows[s - 1] not in (0, 1):
            return 'row of segment {} is {} and follows {}: the rows are non-decreasing and none is without a segment'.format(
                s, rows[s], rows[s - 1]), None, None
    if rows[-1] != B - 1:
        return 'row of segment {} is {}: the last row is B - 1 = {}'.format(S - 1, rows[-1], B - 1), None, None
    n_out, counts = [0] * B, []
    for s, (row, first, frames, pause, step, gain) in enumerate(segments):
        if frames < 0 or pause < 0:
            return 'segment {} has a negative length (frames {}, pause {})'.format(s, frames, pause), None, None
        if frames > 0 and pause > 0:
            return 'segment {} is both speech ({} frames) and a pause ({} frames)'.format(s, frames, pause), None, None
        if frames == 0 and pause == 0:
            return 'segment {} is neither speech nor a pause (frames and pause are 0)'.format(s), None, None
        c = pause
        if frames > 0:
            if first < 0 or first + frames > nf[row]:
                return 'segment {} reads frames {} .. {} of row {}, which has 0 .. {}'.format(s, first, first + frames - 1, row, nf[row] - 1), None, None
            if not STEP_MIN <= step <= STEP_MAX:
                return 'segment {} has step {}, which is not in {} .. {}'.format(s, step, STEP_MIN, STEP_MAX), None, None
            g = np.float32(gain)
            if not (g >= 0 and g <= GAIN_MAX):
                return 'segment {} has a gain that is not finite or lies outside 0 .. 16'.format(s), None, None
            c = count(frames, step)
        counts.append(c)
        n_out[row] += c
    return None, n_out, counts


def room(n_out, T_out):
    """the refusal of a T_out behind a legal list, or None"""
    for b, n in enumerate(n_out):
        if n > T_out:
            return 'T_out = {} is below n_out[{}] = {}'.format(T_out, b, n)
    if T_out > MAX_T_OUT:
        return 'T_out = {} is above 2^30 = {}'.format(T_out, MAX_T_OUT)
    return None


def launches(S):
    return -(-S // SEGMENTS_PER_LAUNCH)


def cut(segments, counts, T_out):
    """The tiles of every launch: a list (one per launch) of lists (one per segment) of the tiles the segment owns -- a segment owns
    its own output frames, a row's last segment everything up to T_out"""
    out, o = [], 0
    for s, q in enumerate(segments):
        last = s + 1 == len(segments) or segments[s + 1][0] != q[0]
        span = T_out - o if last else counts[s]
        if s % SEGMENTS_PER_LAUNCH == 0:
            out.append([])
        out[-1].append(-(-span // TILE))
        o = 0 if last else o + counts[s]
    return out


def blend_segment(x, n, first, c, step, gain):
    """x (F, T) float32 of which n frames may be read -> (F, c) float32: output frame j of a speech segment"""
    x = np.asarray(x, dtype=np.float32)
    F = x.shape[0]
    xp = np.zeros((F, n + 1), np.float64)       # (frame n reads as 0.0)
    xp[:, :n] = x[:, :n]
    p = np.arange(c, dtype=np.int64) * np.int64(step)
    i = first + (p >> 16)
    a = (p & 65535).astype(np.float64) * 2.0 ** -16
    g = np.float64(np.float32(gain))
    with np.errstate(invalid='ignore', over='ignore'):
        t0 = (1.0 - a)[None, :] * xp[:, i]
        t1 = a[None, :] * xp[:, i + 1]
        return (g * (t0 + t1)).astype(np.float32)


def warp(x, segments, n_frames=None, T_out=None):
    """x (B, F, T) float32 -> ``(out (B, F, T_out) float32, n_out)``; T_out None: the longest row"""
    x = np.asarray(x, dtype=np.float32)
    B, F, T = x.shape
    why, n_out, counts = plan(segments, B, T, n_frames)
    assert why is None, why
    T_out = max(n_out) if T_out is None else T_out
    assert room(n_out, T_out) is None
    nf = [T] * B if n_frames is None else [int(v) for v in n_frames]
    out = np.zeros((B, F, T_out), np.float32)
    o = [0] * B
    for (row, first, frames, _pause, step, gain), c in zip(segments, counts):
        if frames > 0:
            out[row, :, o[row]:o[row] + c] = blend_segment(x[row], nf[row], first, c, step, gain)
        o[row] += c
    assert o == n_out
    return out, n_out
