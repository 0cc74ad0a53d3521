"""The inputs the DTW tests share (tests/test_dtw_host.py on the oracle alone, tests/test_gpu_dtw.py against the kernel): float32
feature sequences by name, small enough for the sequential oracle.  ``LARGE`` is the one shape only the vectorised oracle takes."""
import numpy as np

TIE_SEEDS = (0, 1, 2, 3)
TIE_SHAPE = (40, 55)


def ties(seed, na=TIE_SHAPE[0], nb=TIE_SHAPE[1]):
    """few-valued features: D = 2, integers in {0, 1, 2} -- many cells have several best predecessors"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 3, (na, 2)).astype(np.float32)
    b = rng.integers(0, 3, (nb, 2)).astype(np.float32)
    return a, b


def ties_1d(seed, na=TIE_SHAPE[0], nb=TIE_SHAPE[1]):
    """D = 1, integers in {0, 1, 2}: local costs are small integers, so whole sums tie -- seed 1 is a case in which `up` and
    `left` tie below `diagonal`, which the two-dimensional cases above do not contain"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 3, (na, 1)).astype(np.float32)
    b = rng.integers(0, 3, (nb, 1)).astype(np.float32)
    return a, b


def tie_cases():
    """name -> (a, b, D) of every tie case"""
    cases = {}
    for seed in TIE_SEEDS:
        cases['ties seed {}'.format(seed)] = ties(seed) + (2,)
        cases['ties D=1 seed {}'.format(seed)] = ties_1d(seed) + (1,)
    return cases


def random_pair(seed, na, nb, K):
    """cepstrum-like rows: a random walk in time, so that the path wanders off the diagonal"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.standard_normal((na, K)), axis=0).astype(np.float32)
    b = np.cumsum(rng.standard_normal((nb, K)), axis=0).astype(np.float32)
    return a, b


def warped_pair(seed, na, nb, K):
    """b is a time-warped, noisy copy of a: the path has long runs in all three directions"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.standard_normal((na, K)), axis=0).astype(np.float32)
    pos = np.sort(rng.random(nb)) * (na - 1)
    b = (a[np.round(pos).astype(int)] + 0.05 * rng.standard_normal((nb, K))).astype(np.float32)
    return a, b


def shapes(tile):
    """(na, nb) of the GPU comparison: degenerate tables, odd sizes, and the kernel's cut from both sides"""
    return [(1, 1), (1, 9), (9, 1), (37, 53), (53, 37), (tile - 1, tile + 1), (tile, tile), (tile + 1, tile - 1), (2 * tile + 3, tile + 5)]


def host_cases():
    """name -> (a, b, D): every case the two forms of the oracle are held equal on"""
    cases = {}
    for na, nb in [(1, 1), (1, 9), (9, 1), (2, 2), (37, 53), (53, 37)]:
        cases['random {}x{}'.format(na, nb)] = random_pair(na * 100 + nb, na, nb, 13) + (13,)
    cases['warped 60x45'] = warped_pair(5, 60, 45, 5) + (5,)
    cases['D=1'] = random_pair(6, 31, 29, 1) + (1,)
    cases['leading D of wider rows'] = random_pair(7, 23, 34, 9) + (4,)
    cases.update(tie_cases())
    a, b = random_pair(8, 25, 30, 3)
    a[7, 1] = np.nan
    cases['a NaN frame in a'] = (a, b, 3)
    a, b = ties(9, 20, 20)
    b[11, 0] = np.nan
    cases['a NaN frame in b, with ties'] = (a, b, 2)
    a, b = random_pair(10, 12, 14, 2)
    a[3, 0] = np.inf
    cases['an Inf'] = (a, b, 2)
    cases['identical'] = (cases['warped 60x45'][0], cases['warped 60x45'][0].copy(), 5)
    return cases


LARGE = (2048, 2048, 13)
