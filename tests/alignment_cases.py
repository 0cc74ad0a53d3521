"""Inputs of the attention-diagnostics tests (a plain helper module, imported like loudness_cases.py): hand-written utterances whose
records are written out literally, random alignment histories an utterance of which depends on its own shape alone, the shipped
reference alignment, and a synthetic clean one.  test_alignment_host.py holds the oracle to the literals on exactly what
test_gpu_alignment.py feeds the kernels."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def record(n_sent, n_steps, reached, end_step, backward, max_back, max_jump, longest_stall, after_end, off_text, skipped, focus_sum):
    return dict(n_sent=n_sent, n_steps=n_steps, reached=reached, end_step=end_step, backward=backward, max_back=max_back,
                max_jump=max_jump, longest_stall=longest_stall, after_end=after_end, off_text=off_text, skipped=skipped, reserved=0,
                focus_sum=focus_sum)


def _f(*rows):
    return np.array(rows, dtype=np.float32)


# name -> (rows (S, Ts), N, the record, durations, pos).  Every value is a dyadic fraction: the focus sums are exact.
HAND = {
    # forward one token a step, the last token at the last step
    'clean': (_f([.75, .25, 0, 0], [.25, .5, .25, 0], [0, .25, .75, 0]), 3,
              record(3, 3, 2, 2, 0, 0, 1, 1, 0, 0, 0, 2.0), [1, 1, 1, 0], [0, 1, 2]),
    # a tie goes to the lower index (steps 0 and 2); the last token is never reached
    'tie': (_f([.5, .5, 0, 0], [.25, .5, .25, 0], [0, .375, .375, .25]), 4,
            record(4, 3, 1, -1, 0, 0, 1, 2, 0, 0, 0, 1.375), [1, 2, 0, 0], [0, 1, 1]),
    # a NaN wins the argmax, the first one (step 1: index 1, not 3); the focus sum is NaN
    'first_nan': (_f([.5, .25, .25, 0], [.5, NAN, .25, NAN], [0, .25, .25, .5], [0, 0, .25, .75]), 4,
                  record(4, 4, 3, 2, 0, 0, 2, 1, 0, 0, 1, np.nan), [1, 1, 0, 2], [0, 1, 3, 3]),
    # the last token at step 0: everything behind it is "after the end"
    'end_at_0': (_f([0, .25, .75], [.5, .25, .25], [.25, .5, .25], [0, .25, .75]), 3,
                 record(3, 4, 2, 0, 0, 0, 0, 1, 2, 0, 0, 2.5), [1, 1, 2], [2, 0, 1, 2]),
    # never at the last token: the spoken part is every step
    'no_end': (_f([.75, .25, 0, 0], [.5, .25, .25, 0], [.25, .5, .25, 0]), 4,
               record(4, 3, 1, -1, 0, 0, 1, 2, 0, 0, 0, 1.75), [2, 1, 0, 0], [0, 0, 1]),
    # 0 -> 2 -> 0 -> 1 -> 3: jumps ahead of 2, 1 and 2, one step back by 2
    'backward': (_f([.75, .25, 0, 0], [0, .25, .75, 0], [.5, .25, .25, 0], [.25, .5, .25, 0], [0, 0, .25, .75]), 4,
                 record(4, 5, 3, 4, 1, 2, 2, 1, 0, 0, 0, 3.25), [2, 1, 1, 1], [0, 2, 0, 1, 3]),
    # three steps on token 1
    'stall': (_f([.75, .25, 0], [.25, .5, .25], [.25, .5, .25], [.125, .75, .125], [0, .25, .75]), 3,
              record(3, 5, 2, 4, 0, 0, 1, 3, 0, 0, 0, 3.25), [1, 3, 1], [0, 1, 1, 1, 2]),
    # two tokens and two columns of padding: steps 1 and 2 have their strongest weight on padding, step 3 ties with it (the lower
    # index, inside the sentence, wins).  The spoken part is steps 0 .. 2 -- pos 0, 0, 1 -- hence a stall of 2 and no step back
    'off_text': (_f([.75, .25, 0, 0], [.25, .125, .5, .125], [.125, .25, .125, .5], [.125, .375, .375, .125]), 2,
                 record(2, 4, 1, 2, 0, 0, 1, 2, 0, 2, 0, 1.625), [2, 2, 0, 0], [0, 0, 1, 1]),
}


def hand_batch(names=None, fill=NAN):
    """the hand-written utterances as one ragged batch: (alignments (S_max, B, Ts_max), n_sent, n_steps, names); `fill` is what the
    steps behind an utterance hold (never read), and the columns behind a case's own width hold 0 (they are padding: read for off)"""
    names = list(HAND) if names is None else list(names)
    S_max = max(HAND[n][0].shape[0] for n in names)
    Ts = max(HAND[n][0].shape[1] for n in names)
    ali = np.full((S_max, len(names), Ts), fill, np.float32)
    for b, n in enumerate(names):
        rows = HAND[n][0]
        ali[:rows.shape[0], b, :] = 0
        ali[:rows.shape[0], b, :rows.shape[1]] = rows
    return ali, [HAND[n][1] for n in names], [HAND[n][0].shape[0] for n in names], names


def random_utterance(S, Ts, tag=0):
    """rows (S, Ts) float32 of softmax weights, a function of (S, Ts, tag) alone: a peak that wanders, with ties and flat rows
    among them"""
    rng = np.random.default_rng([S, Ts, tag])
    x = rng.standard_normal((S, Ts)).astype(np.float32)
    centre = np.cumsum(rng.integers(-1, 3, S)) % Ts
    x[np.arange(S), centre] += np.float32(3.0)
    w = np.exp(x - x.max(axis=1, keepdims=True))
    rows = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    for s in range(0, S, 7):               # every seventh row: its maximum twice, the second copy further right
        j = int(np.argmax(rows[s]))
        rows[s, (j + 1 + s) % Ts] = rows[s, j]
    return rows


def random_batch(S, B, Ts, tag=0):
    """(S, B, Ts): utterance b is random_utterance(S, Ts, tag + b)"""
    return np.ascontiguousarray(np.stack([random_utterance(S, Ts, tag + b) for b in range(B)], axis=1))


def ragged_lengths(B, hi, tag):
    """B lengths in 1 .. hi with 1 and hi among them (where B allows)"""
    rng = np.random.default_rng([B, hi, tag])
    n = rng.integers(1, hi + 1, B)
    n[0] = hi
    if B > 1:
        n[-1] = 1
    return [int(v) for v in n]


def fixture():
    """the alignment the reference dumped for its first sentence, as rows (200, 92): flat -- every weight 0.0108 .. 0.0110"""
    a = np.load(os.path.join(GOLD, 'reference_alignments_nancy_1.npz'))['alignments']   # (1, Ts, S)
    return np.ascontiguousarray(a[0].T)


MONOTONE = dict(S=40, N=17, Ts=24, width=0.5, speed=0.55)


def monotone():
    """a clean synthetic alignment: gaussian rows of width 0.5 over the N = 17 tokens of Ts = 24, the centre walking 0.55 positions
    a step and resting on the last token; rows (40, 24), N"""
    m = MONOTONE
    j = np.arange(m['N'], dtype=np.float64)
    rows = np.zeros((m['S'], m['Ts']), np.float32)
    for s in range(m['S']):
        c = min(m['speed'] * s, m['N'] - 1.0)
        w = np.exp(-0.5 * ((j - c) / m['width']) ** 2)
        rows[s, :m['N']] = (w / w.sum()).astype(np.float32)
    return rows, m['N']
