"""Case table and inputs of the GEMM tests (a plain helper module, imported like parity.py): shared by the host tests
of the model (tests/test_gemm_model_host.py) and the GPU tests (tests/test_gpu_gemm.py), so that what the host shows about
an input -- a lost product lies far above the bound -- is shown about the very input the GPU sees."""
import numpy as np

import gemm_model as G

# (B, T, Cin, ktaps, N, pool): each the smallest shape that takes the path it names
CASES = [
    (3, 50, 128, 1, 256, 0),        # plain dense, M = 150 (two M tiles, one partly empty)
    (2, 77, 256, 3, 80, 0),         # conv3, N not a multiple of the tile, tap-inner k order (256 % 32 == 0)
    (2, 77, 256, 3, 128, 1),        # ... with the max-pool loader
    (4, 40, 80, 5, 128, 0),         # channel count not a multiple of the tile depth: linear k order
    (5, 30, 2048, 3, 128, 1),       # K = 6144: the split-K shape of the encoder's first projection
    (9, 150, 128, 1, 1025, 0),      # 11 M tiles x 9 N tiles: exercises the XCD tile map with padding
    (1, 1, 4, 1, 1, 0),             # K smaller than one tile, M = N = 1
    (2, 33, 80, 1, 33, 0),          # K = 80 not a multiple of 32, N and M edge blocks
    (3, 21, 128, 2, 96, 0),         # uniform tap-inner, even taps (asymmetric SAME padding)
    (3, 21, 128, 16, 96, 0),        # ... the widest kernel of the tap masks
    (2, 33, 80, 4, 33, 0),          # per-thread tap path, even taps
    (2, 9, 80, 16, 64, 0),          # per-thread tap path, T < ktaps
    (2, 40, 128, 17, 64, 0),        # more than 16 taps: the general path with its division
    (2, 40, 80, 18, 64, 0),         # ... with tiles that straddle taps
    (5, 1, 128, 3, 64, 1),          # pool fast path, sequence ends inside a thread's four rows: T = 1
    (4, 2, 128, 3, 64, 1),          # ... T = 2
    (3, 3, 128, 3, 64, 1),          # ... T = 3
    (7, 5, 128, 3, 64, 1),          # ... T = 5
    (2, 64, 128, 3, 64, 1),         # pool fast path, M exactly one tile
    (3, 43, 128, 3, 64, 1),         # ... one tile plus a row
    (2, 41, 80, 3, 64, 1),          # pool general path: Cin % 32 != 0
    (2, 41, 128, 5, 64, 1),         # pool general path: more than 3 taps
    (2, 20, 1376, 3, 64, 0),        # split-K, K = 4128 = 129 tiles: slices start at tiles 16, 32 (tap 1, 2 of their group)
    (2, 20, 1376, 3, 64, 1),        # ... with the max-pool loader
    (2, 20, 1028, 4, 64, 0),        # split-K on the per-thread path, K = 4112: a partial last tile
    (1, 70, 4096, 1, 40, 0),        # split-K at exactly the threshold
    (1, 24, 256, 17, 32, 0),        # split-K on the general path
]
LEGACY = CASES[:6]
FAMILIES = ('gauss', 'positive')


def case_id(c):
    return 'B{}-T{}-C{}-k{}-N{}-p{}'.format(*c)


def seed_of(case):
    B, T, Cin, ktaps, N, pool = case
    return ((B * 1000 + Cin) * 64 + ktaps) * 4096 + T * 8 + N % 8 + pool * 4


def raised(case):
    """Does the 'positive' family of this case get its low significand bits raised?  One accumulator that takes 768 k or
    more of one-signed products (no split-K) rounds some 300 times at a growing magnitude: the documented arithmetic's own
    worst element, a 4.7 sigma draw among 10^4 outputs, reaches 15 ... 32 u there, and the systematic 120 ... 150 u of a lost
    hi*lo / lo*hi / mid*mid is then less than 8 times as much (measured: 4.6 ... 9.6).  With the low 16 bits of every
    operand set, mid and lo are at the top of their ranges and a lost product costs 350 ... 570 u: 14 times or more."""
    B, T, Cin, ktaps, N, pool = case
    K = Cin * ktaps
    return K >= 768 and G.splitk_slices(K) == 1


def data(case, family):
    """x [B*T][Cin] ~ N(0, 1), w [N][ktaps*Cin] ~ 0.05 N(0, 1), float32; 'positive': the absolute values of the same draws
    (post-relu activations against one-signed weights: the split's one-sided truncation errors add up), with the low
    16 bits set where `raised` says so."""
    B, T, Cin, ktaps, N, pool = case
    rng = np.random.default_rng(seed_of(case))
    x = rng.standard_normal((B * T, Cin)).astype(np.float32)
    w = (rng.standard_normal((N, ktaps * Cin)) * 0.05).astype(np.float32)
    if family == 'positive':
        x, w = np.abs(x), np.abs(w)
        if raised(case):
            x, w = ((v.view(np.uint32) | np.uint32(0xFFFF)).view(np.float32) for v in (x, w))
    return x, w


def full_significands(rng, shape):
    """float32 with all 24 significand bits in play (the last one set), |v| in [0.5, 2), random sign: hi, mid and lo
    of the split are all non-zero."""
    mant = rng.integers(0, 1 << 22, shape, dtype=np.int64) * 2 + 1 + (1 << 23)      # odd, 24 bits
    v = mant.astype(np.float64) * 2.0 ** -23 * 2.0 ** rng.integers(-1, 1, shape)
    return (v * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def power_of_two(rng, shape):
    return (2.0 ** rng.integers(-3, 4, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def routing_ks(case, rng, limit=512):
    """The k the routing test observes: all of them up to `limit`, else `limit` that include the first and last k of
    every tap, of every split-K slice (in the kernel's k order) and of the last, partial tile."""
    B, T, Cin, ktaps, N, pool = case
    K = Cin * ktaps
    if K <= limit:
        return np.arange(K)
    must = set()
    for t in range(ktaps):
        must.update((t * Cin, t * Cin + Cin - 1))
    order = G.k_order(Cin, ktaps, pool)
    for t0, t1 in G.slice_tiles(K):
        seg = order[t0 * G.BK:t1 * G.BK]
        seg = seg[seg >= 0]
        must.update((int(seg[0]), int(seg[-1])))
    last = order[-G.BK:]
    last = last[last >= 0]
    must.update((int(last[0]), int(last[-1]), K - 1))
    rest = np.setdiff1d(np.arange(K), np.fromiter(must, int))
    pick = rng.choice(rest, limit - len(must), replace=False)
    return np.sort(np.concatenate([np.fromiter(must, int), pick]))


def routing_inputs(case):
    """A with full significands, row n of W = +-2^s at one k_n: every output is one operand times a power of two, exact
    in any order of the six products and through max-pool and split-K.  W has max(N, number of observed k) rows."""
    B, T, Cin, ktaps, N, pool = case
    rng = np.random.default_rng(seed_of(case) + 1)
    x = full_significands(rng, (B * T, Cin))
    ks = routing_ks(case, rng)
    Nr = max(N, len(ks))
    w = np.zeros((Nr, ktaps * Cin), np.float32)
    w[np.arange(Nr), ks[np.arange(Nr) % len(ks)]] = power_of_two(rng, Nr)
    return x, w


def mirror_inputs(case):
    """The mirror image for the terms of W (pool = 0 only): W with full significands, A zero but for one +-2^s per row
    with t % ktaps == 0 -- the taps of two such rows never meet in one output, so each output has at most one term."""
    B, T, Cin, ktaps, N, pool = case
    assert not pool
    rng = np.random.default_rng(seed_of(case) + 2)
    w = full_significands(rng, (N, ktaps * Cin))
    x = np.zeros((B * T, Cin), np.float32)
    rows = np.flatnonzero(np.arange(B * T) % T % ktaps == 0)
    x[rows, rng.integers(0, Cin, len(rows))] = power_of_two(rng, len(rows))
    return x, w


def counting_inputs(case):
    """Integers: A in [-127, 127], W in [-8, 8] -- bf16-exact (mid = lo = 0), every partial sum an integer below 2^23 up to
    K = 6144, so the result is the int64 product exactly whatever the order."""
    B, T, Cin, ktaps, N, pool = case
    assert 127 * 8 * Cin * ktaps < 2 ** 23
    rng = np.random.default_rng(seed_of(case) + 3)
    x = rng.integers(-127, 128, (B * T, Cin)).astype(np.float32)
    w = rng.integers(-8, 9, (N, ktaps * Cin)).astype(np.float32)
    return x, w
