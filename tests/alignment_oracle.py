"""The alignment statistics of include/sstts_hip.h (tts_alignment_stats) restated step by step in numpy: a plain sequential walk, one
utterance at a time, with np.argmax for the positions and Python / numpy float64 additions for the focus sum.  What the kernels
return is held to this bit for bit.  A plain helper module (imported like dtw_oracle.py); no GPU, no library."""
import numpy as np

FIELDS = ('n_sent', 'n_steps', 'reached', 'end_step', 'backward', 'max_back', 'max_jump', 'longest_stall', 'after_end', 'off_text',
          'skipped', 'reserved')
# the record as the library lays it out: twelve int32, then one double -- 56 bytes
RECORD = np.dtype([(name, np.int32) for name in FIELDS] + [('focus_sum', np.float64)])
assert RECORD.itemsize == 56


def positions(rows, N):
    """(pos int32 (S,), peak float32 (S,), off int32 (S,)) of the rows (S, Ts) of one utterance with N tokens: np.argmax over the
    sentence (the lowest index of the maximum, the first NaN if there is one), the element there, and whether the argmax of the
    whole padded row lies on padding"""
    rows = np.asarray(rows, dtype=np.float32)
    S = rows.shape[0]
    pos = np.zeros(S, np.int32)
    peak = np.zeros(S, np.float32)
    off = np.zeros(S, np.int32)
    for s in range(S):
        pos[s] = int(np.argmax(rows[s, :N]))
        peak[s] = rows[s, pos[s]]
        off[s] = 1 if int(np.argmax(rows[s])) >= N else 0
    return pos, peak, off


def utterance(rows, N, Ts=None):
    """(record: dict, durations int32 (Ts,), pos, peak) of one utterance: ``rows`` (S, Ts) are its S steps"""
    rows = np.asarray(rows, dtype=np.float32)
    S = rows.shape[0]
    Ts = rows.shape[1] if Ts is None else Ts
    pos, peak, off = positions(rows, N)
    durations = np.zeros(Ts, np.int32)
    end_step = -1
    for s in range(S):
        durations[pos[s]] += 1
        if end_step < 0 and pos[s] == N - 1:
            end_step = s
    E = end_step if end_step >= 0 else S - 1
    backward = max_back = max_jump = 0
    longest = run = 1
    for s in range(1, E + 1):
        d = int(pos[s]) - int(pos[s - 1])
        backward += d < 0
        max_back = max(max_back, -d)
        max_jump = max(max_jump, d)
        run = run + 1 if d == 0 else 1
        longest = max(longest, run)
    after_end = 0 if end_step < 0 else int(sum(1 for s in range(end_step + 1, S) if pos[s] != N - 1))
    reached = int(pos.max())
    focus = np.float64(peak[0])
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(1, S):
            focus = focus + np.float64(peak[s])
    rec = dict(n_sent=int(N), n_steps=int(S), reached=reached, end_step=int(end_step), backward=int(backward), max_back=int(max_back),
               max_jump=int(max_jump), longest_stall=int(longest), after_end=after_end, off_text=int(off.sum()),
               skipped=int(np.sum(durations[:reached] == 0)), reserved=0, focus_sum=np.float64(focus))
    return rec, durations, pos, peak


def batch(alignments, n_sent=None, n_steps=None):
    """``alignments`` (n_steps_max, B, Ts) -> (records: RECORD array (B,), durations int32 (B, Ts), pos int32 (B, n_steps_max) with
    -1 behind an utterance's steps, peak float32 (B, n_steps_max) with 0 there)"""
    alignments = np.asarray(alignments, dtype=np.float32)
    S_max, B, Ts = alignments.shape
    n_sent = [Ts] * B if n_sent is None else list(n_sent)
    n_steps = [S_max] * B if n_steps is None else list(n_steps)
    records = np.zeros(B, RECORD)
    durations = np.zeros((B, Ts), np.int32)
    pos = np.full((B, S_max), -1, np.int32)
    peak = np.zeros((B, S_max), np.float32)
    for b in range(B):
        rec, durations[b], p, k = utterance(alignments[:n_steps[b], b], n_sent[b])
        for name, value in rec.items():
            records[name][b] = value
        pos[b, :n_steps[b]] = p
        peak[b, :n_steps[b]] = k
    return records, durations, pos, peak


def same_records(got, want):
    """the records agree bit for bit: every integer, and the focus sum as a bit pattern (any NaN equals any NaN: the payload of
    a NaN sum is not part of the definition)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    for name in FIELDS:
        if not np.array_equal(got[name], want[name]):
            return False
    g, w = got['focus_sum'], want['focus_sum']
    both_nan = np.isnan(g) & np.isnan(w)
    return bool(np.all(both_nan | (g.view(np.uint64) == w.view(np.uint64))))


def text_lengths(ids, pad_id=0):
    """tts_text_lengths: 1 + the largest j with ids[b][j] != pad_id, 1 for a row of padding"""
    ids = np.asarray(ids)
    out = np.ones(ids.shape[0], np.int32)
    for b in range(ids.shape[0]):
        nz = np.flatnonzero(ids[b] != pad_id)
        if nz.size:
            out[b] = nz[-1] + 1
    return out
