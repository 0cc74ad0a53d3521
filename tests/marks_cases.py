"""Inputs of the timing-mark tests (a plain helper module, imported like alignment_cases.py): the planted staircase with its
outlier rows, alignment histories of every kind the weight rule tells apart, and the shapes the GPU tests run -- an utterance
depends on its own shape and tag alone."""
import numpy as np

import alignment_cases as AC

fixture = AC.fixture
ragged_lengths = AC.ragged_lengths

STAIRCASE = dict(S=40, N=23, J=3)


def staircase(rng, S=40, N=23, J=3, outliers=4):
    """(rows float32 (S, N), true int64 (S,)): the true token advances by 0 .. J a step from token 0 at step 0; a row is 0.4 *
    noise / its sum plus 0.6 on the true token, and ``outliers`` rows behind step 4 carry a 0.9 five tokens BACK"""
    steps = rng.integers(0, J + 1, size=S)
    steps[0] = 0
    true = np.minimum(np.cumsum(steps), N - 1)
    rows = rng.random((S, N)).astype(np.float32)
    rows = 0.4 * rows / rows.sum(1, keepdims=True)
    rows[np.arange(S), true] += 0.6
    if S > 5 and outliers:
        for s in rng.choice(np.arange(5, S), min(outliers, S - 5), replace=False):
            rows[s, max(0, true[s] - 5)] = 0.9
    return rows.astype(np.float32), true


KINDS = ('staircase', 'uniform', 'equal', 'zero', 'special')
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -0.25, -3e38, 1e-45, 1e-39, -1e-40, 1.1754942e-38], np.float32)


def utterance(kind, S, Ts, tag=0):
    """rows (S, Ts) float32, a function of (kind, S, Ts, tag) alone"""
    rng = np.random.default_rng([KINDS.index(kind), S, Ts, tag])
    if kind == 'staircase':
        return staircase(rng, S, Ts, 3)[0]
    if kind == 'uniform':
        return rng.random((S, Ts)).astype(np.float32)
    if kind == 'equal':
        return np.full((S, Ts), 0.25, np.float32)
    if kind == 'zero':
        return np.zeros((S, Ts), np.float32)
    rows = AC.random_utterance(S, Ts, tag)          # softmax rows with ties, a tenth of the elements special values
    hit = rng.random((S, Ts)) < 0.1
    rows[hit] = SPECIALS[rng.integers(0, len(SPECIALS), int(hit.sum()))]
    return rows


def batch(kind, S, B, Ts, tag=0):
    """(S, B, Ts): utterance b is utterance(kind, S, Ts, tag + b); kind 'mixed': the kinds in turn"""
    kinds = [KINDS[b % len(KINDS)] if kind == 'mixed' else kind for b in range(B)]
    return np.ascontiguousarray(np.stack([utterance(kinds[b], S, Ts, tag + b) for b in range(B)], axis=1))


# (S, B, Ts, J) of the oracle comparison: every S of 1, 2, 63, 64, 65, 130; every Ts of 1, 2, 63, 64, 65, 130 and 300 -- above the
# 256 columns one pass of the lanes covers --; B of 1, 3 and 65 (a second launch's lengths); J of 1, 2 and 15.  130 x 130 keeps its
# directions in LDS, 130 x 300 does not.
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 2), (63, 1, 64, 15), (64, 3, 63, 1), (65, 3, 65, 2), (130, 1, 130, 15), (130, 3, 300, 2), (2, 65, 63, 1),
          (1, 3, 300, 15), (65, 1, 2, 1), (64, 1, 1, 2), (5, 65, 130, 15)]
