"""The DTW oracle on the CPU (tests/dtw_oracle.py): its two forms agree bit for bit on every shared case, the results have the
properties the header states, and the tie rule is visible in them -- so the GPU comparison of tests/test_gpu_dtw.py really holds
the kernel to that rule.  No GPU."""
import numpy as np
import pytest

import dtw_cases as K
import dtw_oracle as W

CASES = K.host_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_two_forms_of_the_oracle_agree(name):
    a, b, D = CASES[name]
    cost, plen, path = W.dtw_sequential(a, b, D)
    cost2, plen2, path2 = W.dtw_diagonals(a, b, D)
    assert W.same_bits(cost, cost2) and plen == plen2 and np.array_equal(path, path2)
    # the path is a monotone chain of single steps from (0, 0) to the last cell, and path_len counts it
    na, nb = a.shape[0], b.shape[0]
    assert plen == len(path) and max(na, nb) <= plen <= na + nb - 1
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (na - 1, nb - 1)
    steps = np.diff(path, axis=0)
    assert set(map(tuple, steps.tolist())) <= {(1, 1), (1, 0), (0, 1)}
    # ... and its cost is the sum of the local costs along it, in path order
    c = W.local_costs(a, b, D)
    total = c[0, 0]
    for i, j in path[1:]:
        total = c[i, j] + total
    assert W.same_bits(total, cost)
    assert np.isnan(cost) == bool(np.isnan(a[:, :D]).any() or np.isnan(b[:, :D]).any())


def test_identical_sequences_cost_nothing_along_the_diagonal():
    a, b, D = CASES['identical']
    cost, plen, path = W.dtw_sequential(a, b, D)
    assert cost == 0.0 and plen == a.shape[0] and np.array_equal(path[:, 0], path[:, 1])


def test_the_tie_rule_moves_the_path_length():
    """few-valued features: the order of the candidates decides path_len (the cost is the same minimum either way)"""
    ours, other = [], []
    for seed in K.TIE_SEEDS:
        a, b = K.ties(seed)
        cost, plen, path = W.dtw_sequential(a, b, 2)
        cost2, plen2, path2 = W.dtw_sequential(a, b, 2, order=(W.UP, W.LEFT, W.DIAG))
        assert W.same_bits(W.dtw_diagonals(a, b, 2, order=(W.UP, W.LEFT, W.DIAG))[0], cost2)
        assert cost == cost2 and not np.array_equal(W.padded_path(path, 94), W.padded_path(path2, 94))
        ours.append(plen)
        other.append(plen2)
    assert ours == [58, 63, 58, 59] and other == [62, 64, 63, 60]
    # every other order of the candidates is told apart on at least one of the tie cases, too
    for order in [(W.DIAG, W.LEFT, W.UP), (W.UP, W.DIAG, W.LEFT), (W.LEFT, W.DIAG, W.UP), (W.LEFT, W.UP, W.DIAG)]:
        differs = False
        for a, b, D in K.tie_cases().values():
            differs |= not np.array_equal(W.dtw_diagonals(a, b, D)[2], W.dtw_diagonals(a, b, D, order=order)[2])
        assert differs, order


def test_a_strict_comparison_is_part_of_the_rule():
    """'replaces iff strictly smaller': with <= the later candidate wins a tie, which the tie cases tell apart"""
    a, b = K.ties(0)
    c = W.local_costs(a, b, 2)
    na, nb = c.shape
    Dm = np.zeros((na, nb))
    L = np.zeros((na, nb), int)
    for i in range(na):
        for j in range(nb):
            cands = [(Dm[i - 1, j - 1], L[i - 1, j - 1]) if i and j else None, (Dm[i - 1, j], L[i - 1, j]) if i else None,
                     (Dm[i, j - 1], L[i, j - 1]) if j else None]
            best = None
            for cand in cands:
                if cand is not None and (best is None or cand[0] <= best[0]):
                    best = cand
            Dm[i, j], L[i, j] = (c[i, j] + best[0], best[1] + 1) if best else (c[0, 0], 1)
    assert Dm[-1, -1] == W.dtw_sequential(a, b, 2)[0] and L[-1, -1] != W.dtw_sequential(a, b, 2)[1]


def test_only_the_first_D_floats_and_the_frames_given_count():
    a, b, D = CASES['leading D of wider rows']
    ref = W.dtw_sequential(a, b, D)
    a2, b2 = a.copy(), b.copy()
    a2[:, D:] = np.nan
    b2[:, D:] = 7.0
    got = W.dtw_sequential(a2, b2, D)
    assert W.same_bits(ref[0], got[0]) and np.array_equal(ref[2], got[2])
