"""CPU: the oracle of the monotonic alignment search (tests/marks_oracle.py) held to what defines it -- the largest sum over every
legal path by enumeration, the legality of its own path, the tie rules -- and to the planted staircase it has to find.  What the
kernel is compared with (tests/test_gpu_token_times.py) is therefore right before a GPU is asked."""
import numpy as np

import marks_cases as C
import marks_oracle as O


def test_the_score_is_the_brute_force_maximum_and_the_path_earns_it():
    rng = np.random.default_rng(0)
    for trial in range(300):
        S, N, J = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 3))
        rows = rng.random((S, N)).astype(np.float32)
        if trial % 3 == 0:
            rows = (np.round(rows * 2) / 2).astype(np.float32)      # 0, 0.5 and 1: ties
        rec, start, q = O.utterance(rows, N, J)
        w = O.weights(rows)
        assert rec['score'] == O.brute(rows, N, J) == sum(int(w[s, q[s]]) for s in range(S)), trial
        assert O.legal(q, N, J) and q[-1] == rec['last'], trial
        # start telescopes to S: the durations of the tokens are the steps
        assert start[0] == 0 and start[N] == S and np.all(np.diff(start) >= 0), trial
        assert [int(start[j + 1] - start[j]) for j in range(N)] == [int(np.sum(q == j)) for j in range(N)], trial
        assert rec['skipped'] == sum(1 for j in range(rec['last']) if not np.any(q == j)), trial


def test_the_planted_staircase_comes_back():
    rng = np.random.default_rng(0)
    m = C.STAIRCASE
    for trial in range(50):
        rows, true = C.staircase(rng)
        rec, _start, q = O.utterance(rows, m['N'], m['J'])
        assert np.array_equal(q, true), trial
        assert rec['agree'] == 36 and O.reliable(rec), trial        # the four outlier rows: the argmax stands five tokens back


def test_the_tie_rules_on_equal_and_zero_rows():
    for value in (0.25, 0.0):
        rows = np.full((7, 9), value, np.float32)
        rec, start, q = O.utterance(rows, 9, 3)
        assert not q.any() and rec['last'] == 0 and rec['jumps'] == 0 and rec['skipped'] == 0 and rec['agree'] == 7
        assert rec['score'] == 7 * int(np.float32(value).view(np.uint32))
        assert start[0] == 0 and np.all(start[1:] == 7)
    # the smallest d: two equal ways into the last cell, from the same token and from the one before
    rows = np.array([[.5, .5, 0], [0, .5, 0]], np.float32)
    assert list(O.utterance(rows, 3, 1)[2]) == [1, 1]
    # the lowest last column: tokens 1 and 2 end on the same sum
    rows = np.array([[.5, .5, 0], [0, .5, .5]], np.float32)
    assert list(O.utterance(rows, 3, 1)[2]) == [1, 1]


def test_the_weight_rule():
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-45, 1.0, 0.5], np.float32)
    assert list(O.weights(x)) == [0, 0x7f800000, 0, 0, 0, 0, 1, 0x3f800000, 0x3f000000]
    # a monotone piecewise-linear log2 scaled by 2^23, at most 0.086 octave off
    v = np.linspace(1.0, 2.0, 1001).astype(np.float32)
    err = (O.weights(v) - 0x3f800000) / 2.0 ** 23 - np.log2(v.astype(np.float64))
    assert np.all(np.diff(O.weights(v)) >= 0) and 0.0860 < np.abs(err).max() < 0.0861


def test_counts_on_a_hand_case():
    # tokens 0, 0, 2, 2, 5 with J = 3: jumps at steps 2 and 4, tokens 1, 3 and 4 skipped
    rows = np.zeros((5, 7), np.float32)
    for s, j in enumerate((0, 0, 2, 2, 5)):
        rows[s, j] = 1.0
    rec, start, q = O.utterance(rows, 6, 3, Ts=7)
    assert list(q) == [0, 0, 2, 2, 5] and rec['jumps'] == 2 and rec['skipped'] == 3 and rec['last'] == 5 and rec['agree'] == 5
    assert list(start) == [0, 2, 2, 4, 4, 4, 5, 5]
    # the first step may stand up to J tokens in: a jump where it is more than one
    rows = np.zeros((2, 4), np.float32)
    rows[0, 2] = rows[1, 3] = 1.0
    rec, start, q = O.utterance(rows, 4, 2)
    assert list(q) == [2, 3] and rec['jumps'] == 1 and rec['skipped'] == 2 and list(start) == [0, 0, 0, 1, 2]


def test_the_reference_alignment_is_monotone_and_not_reliable():
    rows = C.fixture()
    start, stats, path = O.batch(rows[:, None, :], [92], None, 4)
    assert np.all(np.diff(path[0]) >= 0) and np.all(np.diff(path[0]) <= 4)
    assert start[0, 0] == 0 and start[0, 92] == 200 and not O.reliable(stats[0])


def test_batches_are_utterances():
    ali = C.batch('mixed', 9, 5, 11)
    n_sent, n_steps = [11, 1, 5, 7, 11], [9, 9, 1, 4, 2]
    start, stats, path = O.batch(ali, n_sent, n_steps, 2)
    for b in range(5):
        rec, st, q = O.utterance(ali[:n_steps[b], b], n_sent[b], 2)
        assert np.array_equal(start[b], st) and np.array_equal(path[b, :n_steps[b]], q) and np.all(path[b, n_steps[b]:] == -1)
        assert all(stats[name][b] == value for name, value in rec.items())
        assert np.all(start[b, n_sent[b]:] == n_steps[b])
