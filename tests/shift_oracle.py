"""Oracle of the formant-preserving pitch stage (tts_shift_magnitudes): a from-scratch numpy restatement in float64 of the formulas
include/sstts_hip.h states, plus the plan -- the checks of a segment list in the library's order with the library's words, and
the cut into launches and tiles.  A segment is a row ``(row, first, frames, pitch_step, formant_step)``, or six fields with
``reserved`` in fourth place.

The arithmetic can also be run in float32 (``dtype=np.float32``), with its sums reversed (``reverse=True``) or with the lifter's
last coefficient dropped (``drop_last=True``): the variants the bound has to tell apart or let pass."""
import numpy as np

UNITY = 65536
STEP_MIN, STEP_MAX = 32768, 131072
MAX_SEGMENTS = 4096
SEGMENTS_PER_LAUNCH = 64
TILE = 8            # tts_shift_tile(): frames of a computed segment per workgroup
COPY_TILE = 64      # frames of a copied run per workgroup
MAX_ORDER = 256
N_MIN, N_MAX = 128, 2048
FLOOR = 1e-10


def step(semitones):
    """floor(65536 * 2 ** (-st / 12) + 0.5)"""
    return int(np.floor(65536.0 * 2.0 ** (-float(semitones) / 12.0) + 0.5))


def bins_n(F):
    N = F - 1
    return N if N_MIN <= N <= N_MAX and N & (N - 1) == 0 else 0


def fields(q):
    """(row, first, frames, reserved, pitch_step, formant_step) of a five- or six-field segment"""
    q = tuple(int(v) for v in q)
    return q if len(q) == 6 else q[:3] + (0,) + q[3:]


def plan(segments, B, F, T, n_frames=None, order=33):
    """None for a legal list, else the refusal in the library's words"""
    S = len(segments)
    if B < 1 or T < 1 or S < 1:
        return 'need B, T, S >= 1'
    N = bins_n(F)
    if not N:
        return 'F = {} is not 2^m + 1 with 2^m in {} .. {}'.format(F, N_MIN, N_MAX)
    order_max = min(MAX_ORDER, N // 2)
    if not 2 <= order <= order_max:
        return 'order = {} is not in 2 .. {}'.format(order, order_max)
    if S > MAX_SEGMENTS:
        return '{} segments are more than tts_shift_max_segments() = {}'.format(S, MAX_SEGMENTS)
    if B > S:
        return '{} rows of {} segments: no row is without a segment'.format(B, S)
    nf = [T] * B if n_frames is None else [int(v) for v in n_frames]
    for b, n in enumerate(nf):
        if not 1 <= n <= T:
            return 'n_frames[{}] = {} is not in 1 .. T = {}'.format(b, n, T)
    seg = [fields(q) for q in segments]
    rows = [q[0] for q in seg]
    if rows[0] != 0:
        return 'row of segment 0 is {}: the rows start at 0'.format(rows[0])
    for s in range(1, S):
        if rows[s] - rows[s - 1] not in (0, 1):
            return 'row of segment {} is {} and follows {}: the rows are non-decreasing and none is without a segment'.format(s, rows[s], rows[s - 1])
    if rows[-1] != B - 1:
        return 'row of segment {} is {}: the last row is B - 1 = {}'.format(S - 1, rows[-1], B - 1)
    prev_end = 0
    for s, (row, first, frames, reserved, ps, fs) in enumerate(seg):
        if s > 0 and rows[s - 1] != row:
            prev_end = 0
        if frames < 1:
            return 'segment {} has {} frames: at least 1 is needed'.format(s, frames)
        if first < 0 or first + frames > nf[row]:
            return 'segment {} covers frames {} .. {} of row {}, which has 0 .. {}'.format(s, first, first + frames - 1, row, nf[row] - 1)
        if first < prev_end:
            return ("segment {} starts at frame {} of row {}, in front of its predecessor's end {}: the ranges of a row ascend and do not "
                    'overlap').format(s, first, row, prev_end)
        if reserved != 0:
            return 'segment {} has reserved = {}, which must be 0'.format(s, reserved)
        if not STEP_MIN <= ps <= STEP_MAX:
            return 'segment {} has pitch_step {}, which is not in {} .. {}'.format(s, ps, STEP_MIN, STEP_MAX)
        if not STEP_MIN <= fs <= STEP_MAX:
            return 'segment {} has formant_step {}, which is not in {} .. {}'.format(s, fs, STEP_MIN, STEP_MAX)
        prev_end = first + frames
    return None


def launches(S):
    return -(-S // SEGMENTS_PER_LAUNCH)


def cut(segments, T):
    """The tiles of every launch: a list (one per launch) of lists (one per segment) of ``(lead, body, rest)`` tiles -- a segment
    owns the uncovered frames in front of it, its own, and as its row's last the row's rest up to T"""
    out, prev_end = [], 0
    seg = [fields(q) for q in segments]
    for s, (row, first, frames, _r, ps, fs) in enumerate(seg):
        if s > 0 and seg[s - 1][0] != row:
            prev_end = 0
        last = s + 1 == len(seg) or seg[s + 1][0] != row
        end = first + frames
        body = COPY_TILE if (ps, fs) == (UNITY, UNITY) else TILE
        if s % SEGMENTS_PER_LAUNCH == 0:
            out.append([])
        out[-1].append((-(-(first - prev_end) // COPY_TILE), -(-frames // body), -(-((T if last else end) - end) // COPY_TILE)))
        prev_end = end
    return out


def cos_table(N):
    """ct[j] = cos(pi j / N), j < 2N"""
    return np.cos(np.pi * np.arange(2 * N, dtype=np.float64) / N)


def lifter(Q, drop_last=False):
    h = 1.0 + np.cos(np.pi * np.arange(Q, dtype=np.float64) / Q)
    h[0] = 1.0
    if drop_last:
        h[Q - 1] = 0.0
    return h


def eta(Q, F, max_abs_log):
    """2^-53 * 8 Q (F + 2) (1 + max |L|): what the double roundings of the two sums, log, exp and the table may add"""
    return 2.0 ** -53 * 8.0 * Q * (F + 2) * (1.0 + max_abs_log)


def envelope(x, Q, dtype=np.float64, reverse=False, drop_last=False):
    """x (F, n) -> ``(E (F, n), max |L| per frame)``: the liftered cepstral envelope of every column, in ``dtype``"""
    x = np.asarray(x).astype(dtype)
    F = x.shape[0]
    N = F - 1
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        L = np.log(np.maximum(x, dtype(FLOOR)))           # (np.maximum hands a NaN on)
        C = cos_table(N)[np.outer(np.arange(F), np.arange(Q)) % (2 * N)].astype(dtype)   # (F, Q)
        w = np.ones(F, dtype)
        w[0] = w[N] = 0.5
        A = w[:, None] * L
        c = (C[::-1].T @ A[::-1] if reverse else C.T @ A) / dtype(N)                        # (Q, n)
        hc = lifter(Q, drop_last).astype(dtype)[:, None] * c
        E = C[:, ::-1] @ hc[::-1] if reverse else C @ hc
        return E, np.abs(L).max(axis=0)


def positions(N, s, fold):
    """(i, i + 1 clipped, a) of every bin k = 0 .. N at step s: folded at Nyquist (the fine structure) or clipped (the envelope)"""
    p = np.arange(N + 1, dtype=np.int64) * np.int64(s)
    nyq = np.int64(N) << 16
    p = np.where(p > nyq, 2 * nyq - p, p) if fold else np.minimum(p, nyq)
    i = p >> 16
    return i, np.minimum(i + 1, N), (p & 65535).astype(np.float64) * 2.0 ** -16


def shift_frames(x, pitch_step, formant_step, Q, dtype=np.float64, reverse=False, drop_last=False):
    """x (F, n) float32, every column a computed frame -> ``(y, spread, max |L|)``: the unrounded result (F, n), |t1| + |t2| of the
    blend's two terms times exp(Ew), and the largest |L| of every frame.  A frame with a NaN or an Inf is all NaN."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[0] - 1
    E, max_l = envelope(x, Q, dtype, reverse, drop_last)
    xd = x.astype(dtype)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        X = xd * np.exp(-E)
        i, i1, a = positions(N, pitch_step, True)
        j, j1, af = positions(N, formant_step, False)
        a, af = a.astype(dtype)[:, None], af.astype(dtype)[:, None]
        g = np.exp((1 - af) * E[j] + af * E[j1])
        t1, t2 = g * ((1 - a) * X[i]), g * (a * X[i1])
        y = g * ((1 - a) * X[i] + a * X[i1])
    bad = ~np.isfinite(x).all(axis=0)
    y[:, bad] = np.nan
    return y, np.abs(t1) + np.abs(t2), max_l


def shift(x, segments, n_frames=None, order=33, **variant):
    """x (B, F, T) float32 -> a dict: ``out`` (B, F, T) float32 (y rounded once; copies and zeros as they are), ``y`` float64 (the
    unrounded result where computed), ``slack`` = eta (|t1| + |t2|) and ``computed`` (B, T), the frames that are neither"""
    x = np.asarray(x, dtype=np.float32)
    B, F, T = x.shape
    why = plan(segments, B, F, T, n_frames, order)
    assert why is None, why
    nf = [T] * B if n_frames is None else [int(v) for v in n_frames]
    out = np.zeros((B, F, T), np.float32)
    y = np.zeros((B, F, T), np.float64)
    slack = np.zeros((B, F, T), np.float64)
    computed = np.zeros((B, T), bool)
    for b in range(B):
        out[b, :, :nf[b]] = x[b, :, :nf[b]]
    for row, first, frames, _r, ps, fs in (fields(q) for q in segments):
        if (ps, fs) == (UNITY, UNITY):
            continue
        sl = slice(first, first + frames)
        v, spread, max_l = shift_frames(x[row, :, sl], ps, fs, order, **variant)
        with np.errstate(invalid='ignore', over='ignore'):
            out[row, :, sl] = v.astype(np.float32)
            y[row, :, sl] = v
            slack[row, :, sl] = eta(order, F, np.where(np.isfinite(max_l), max_l, 0.0))[None, :] * np.where(np.isfinite(spread), spread, 0.0)
        computed[row, sl] = True
    return dict(out=out, y=y, slack=slack, computed=computed)


def excess(got, res):
    """|got - y| / (2^-24 |y| + slack + 2^-150) over the computed, finite elements (B, F, T); 0 elsewhere.  2^-150 is half the
    spacing of float32's denormals: what one rounding to float32 may add where 2^-24 |y| is below it."""
    got = np.asarray(got, dtype=np.float32).astype(np.float64)
    y, mask = res['y'], np.broadcast_to(res['computed'][:, None, :], res['y'].shape) & np.isfinite(res['y'])
    with np.errstate(invalid='ignore'):
        r = np.abs(got - y) / (2.0 ** -24 * np.abs(y) + res['slack'] + 2.0 ** -150)
    return np.where(mask, r, 0.0)


def assert_holds(got_bits, res, what):
    """every copy, zero and NaN position bit for bit; every computed element within the bound"""
    got = got_bits.view(np.float32)
    want = res['out']
    assert got.shape == want.shape, (what, got.shape, want.shape)
    comp = np.broadcast_to(res['computed'][:, None, :], want.shape)
    same = got_bits[~comp] == want.view(np.uint32)[~comp]
    assert same.all(), (what, 'copies and zeros', np.argwhere(~comp)[~same][:5])
    nan = np.isnan(res['y']) & comp
    assert np.array_equal(np.isnan(got) & comp, nan), (what, 'NaN positions', np.argwhere((np.isnan(got) & comp) != nan)[:5])
    zero = comp & (res['y'] == 0) & ~np.signbit(res['y'])
    assert not got_bits[zero].any(), (what, 'zeros of computed frames are +0.0')
    r = excess(got, res)
    assert r.max() <= 1.0, (what, 'bound', float(r.max()), np.unravel_index(r.argmax(), r.shape))
    return float(r.max())
