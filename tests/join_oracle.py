"""Oracle of the join and of the speech interval (a plain helper module; nothing in the package imports it).

``join``: a sequential numpy restatement, in float64, of what include/sstts_hip.h says tts_join computes -- piece by piece and
sample by sample, every operation an individually rounded IEEE double operation (numpy float64 scalars never contract).
``speech_interval_batch``: both ends of the interval tests/eos_oracle.py finds, for a batch.

Everything here is exact: tts_join and tts_speech_interval must give these bits."""
import numpy as np

import eos_oracle as E


def fades(counts, fade):
    """f_p = min(fade, count[p] // 2)"""
    return [min(int(fade), int(c) // 2) for c in counts]


def plan(pieces, groups, fade):
    """``(offsets, n_out, f)`` of a list of ``(row, first, count, gap)`` with its groups (non-decreasing from 0): o of a group's
    first piece is 0, o[p+1] = o[p] + count[p] + gap[p], n_out[g] = o[last] + count[last]; the last gap of a group is ignored."""
    pieces = [tuple(int(v) for v in q) for q in pieces]
    groups = [int(g) for g in groups]
    f = fades([q[2] for q in pieces], fade)
    offsets, n_out, o = [], [0] * (groups[-1] + 1), 0
    for p, (_row, _first, count, gap) in enumerate(pieces):
        offsets.append(o)
        if p + 1 == len(pieces) or groups[p + 1] != groups[p]:
            n_out[groups[p]] = o + count
            o = 0
        else:
            assert -gap <= min(f[p], f[p + 1]), (p, gap, f[p], f[p + 1])
            o += count + gap
    return offsets, n_out, f


def s_curve(t):
    """s(t) = (t * t) * (3.0 - 2.0 * t) on a float64"""
    t = np.float64(t)
    return (t * t) * (np.float64(3.0) - np.float64(2.0) * t)


def gain(i, count, f):
    """the gain of sample i of a piece of ``count`` samples fading over f at either edge: a float64"""
    if i < f:
        return s_curve(np.float64(2 * i + 1) / np.float64(2 * f))
    if i >= count - f:
        return s_curve(np.float64(2 * (count - 1 - i) + 1) / np.float64(2 * f))
    return np.float64(1.0)


def join(wav, pieces, groups, fade, N_out):
    """out (G, N_out) float32 of a float32 batch ``wav`` (B, N).  Per output sample the contributors are collected in the order
    of the list (the earlier piece first): none -> +0.0; one of gain 1 -> the source's bits; one of gain w -> float32(float64(x)
    * w); two -> float32(float64(x_a) * w_a + float64(x_b) * w_b)."""
    wav = np.asarray(wav, dtype=np.float32)
    offsets, n_out, f = plan(pieces, groups, fade)
    G = len(n_out)
    assert max(n_out) <= N_out
    who = [[[] for _ in range(N_out)] for _ in range(G)]
    for p, (row, first, count, _gap) in enumerate(pieces):
        for i in range(int(count)):
            who[int(groups[p])][offsets[p] + i].append((int(row), int(first) + i, gain(i, int(count), f[p])))
    out = np.zeros((G, N_out), dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in range(G):
            for j, c in enumerate(who[g]):
                assert len(c) <= 2
                if len(c) == 1:
                    row, k, w = c[0]
                    out[g, j] = wav[row, k] if w == 1.0 else np.float32(np.float64(wav[row, k]) * w)
                elif len(c) == 2:
                    (ra, ka, wa), (rb, kb, wb) = c
                    out[g, j] = np.float32(np.float64(wav[ra, ka]) * wa + np.float64(wav[rb, kb]) * wb)
    return out, n_out


def speech_interval_batch(spec_btf, threshold):
    """the first and the last active frame of every utterance of a time-major batch (B, T, F), as tts_speech_interval takes it: two
    int32 arrays, -1 where ``eos_oracle.silence_interval`` finds no frame above the threshold"""
    out = [E.silence_interval(np.asarray(u).T, threshold) or (-1, -1) for u in spec_btf]
    return np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32)
