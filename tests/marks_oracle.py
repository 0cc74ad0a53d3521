"""The monotonic alignment search of include/sstts_hip.h (tts_token_times) restated cell by cell in numpy and Python integers: a
plain sequential fill of the table, one utterance at a time, a walk back, and counts.  What the kernel returns is held to this
bit for bit.  ``brute`` states the same maximum by enumerating every legal path.  A plain helper module (imported like
alignment_oracle.py); no GPU, no library."""
import itertools

import numpy as np

import alignment_oracle as A

FIELDS = ('n_sent', 'n_steps', 'last', 'jumps', 'skipped', 'agree')
# the record as the library lays it out: an int64, then six int32 -- 32 bytes
RECORD = np.dtype([('score', np.int64)] + [(name, np.int32) for name in FIELDS])
assert RECORD.itemsize == 32


def weights(rows):
    """w(s, j) int64: the float32 element's own bit pattern where the element is greater than 0, else 0 (NaN, zeros, negatives)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    bits = rows.view(np.uint32).astype(np.int64)
    with np.errstate(invalid='ignore'):
        return np.where(rows > 0, bits, 0)


def table(rows, N, J):
    """(D, d) int64 (S, N): the table -- unreachable cells -1 -- and the step d(s, j) that led into every cell"""
    w = weights(np.asarray(rows, dtype=np.float32)[:, :N])
    S = w.shape[0]
    D = np.full((S, N), -1, np.int64)
    step = np.zeros((S, N), np.int64)
    for j in range(min(J, N - 1) + 1):
        D[0, j] = w[0, j]
    for s in range(1, S):                          # row by row; a row's columns at once, d ascending
        best = np.full(N, -1, np.int64)
        for d in range(min(J, N - 1) + 1):
            cand = np.full(N, -1, np.int64)
            cand[d:] = D[s - 1, :N - d]            # the predecessor j - d of every column j >= d
            better = cand > best                   # strictly: among equal predecessors the smallest d
            best[better] = cand[better]
            step[s, better] = d
        D[s] = np.where(best >= 0, best + w[s], -1)
    return D, step


def utterance(rows, N, J, Ts=None):
    """(record: dict, start int32 (Ts + 1,), path int32 (S,)) of one utterance: ``rows`` (S, Ts) are its S steps"""
    rows = np.asarray(rows, dtype=np.float32)
    S = rows.shape[0]
    Ts = rows.shape[1] if Ts is None else Ts
    D, step = table(rows, N, J)
    last = int(np.argmax(D[S - 1]))               # the lowest column of the maximum
    q = np.zeros(S, np.int64)
    q[S - 1] = last
    for s in range(S - 1, 0, -1):
        q[s - 1] = q[s] - step[s, q[s]]
    start = np.full(Ts + 1, S, np.int32)
    for j in range(N + 1):
        start[j] = int(np.sum(q < j))
    jumps = int(sum(1 for s in range(1, S) if q[s] - q[s - 1] > 1)) + (1 if q[0] > 1 else 0)
    skipped = int(sum(1 for j in range(last) if start[j + 1] == start[j]))
    pos = A.positions(rows, N)[0]
    rec = dict(score=int(D[S - 1, last]), n_sent=int(N), n_steps=int(S), last=last, jumps=jumps, skipped=skipped,
               agree=int(np.sum(q == pos)))
    return rec, start, q.astype(np.int32)


def batch(alignments, n_sent=None, n_steps=None, max_jump=4):
    """``alignments`` (n_steps_max, B, Ts) -> (start int32 (B, Ts + 1), records: RECORD array (B,), path int32 (B, n_steps_max)
    with -1 behind an utterance's steps)"""
    alignments = np.asarray(alignments, dtype=np.float32)
    S_max, B, Ts = alignments.shape
    n_sent = [Ts] * B if n_sent is None else list(n_sent)
    n_steps = [S_max] * B if n_steps is None else list(n_steps)
    records = np.zeros(B, RECORD)
    start = np.zeros((B, Ts + 1), np.int32)
    path = np.full((B, S_max), -1, np.int32)
    for b in range(B):
        rec, start[b], q = utterance(alignments[:n_steps[b], b], n_sent[b], max_jump)
        for name, value in rec.items():
            records[name][b] = value
        path[b, :n_steps[b]] = q
    return start, records, path


def same_records(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and all(np.array_equal(got[name], want[name]) for name in ('score',) + FIELDS)


def legal(q, N, J):
    """the path starts within J of token 0, never goes back, advances by at most J and stays inside the sentence"""
    q = [int(v) for v in q]
    return 0 <= q[0] <= J and all(0 <= b - a <= J for a, b in zip(q[:-1], q[1:])) and q[-1] < N


def brute(rows, N, J):
    """the largest sum of weights over every legal path, by enumeration (small tables only)"""
    w = weights(np.asarray(rows, dtype=np.float32)[:, :N])
    S = w.shape[0]
    best = -1
    for p in itertools.product(range(N), repeat=S):
        if legal(p, N, J):
            best = max(best, sum(int(w[s, p[s]]) for s in range(S)))
    return best


def reliable(record):
    """tacotron.marks.reliable restated: the path stands on the argmax at half of the steps or more"""
    return int(record['agree']) * 2 >= int(record['n_steps'])
