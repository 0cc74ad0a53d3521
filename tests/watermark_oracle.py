"""The audio watermark (csrc/watermark_plan.h, include/sstts_hip.h) as plain numpy, operation by operation: the keyed carrier, the
block envelope, the embedder in individually rounded float64 operations with one rounding to float32, and the detector twice --
``detect_brute``, the definition sample by sample and offset by offset (N D work), and ``detect``, the chip-sum form the device
runs (chip sums once a phase, cross-correlated with the signs: N D / L).  Every sum of the detector is an integer sum; where a
float64 ``bincount`` carries one its size is far below 2^53, so it is exact.  No GPU, no library."""
import collections
import math

import numpy as np

BLOCK = 64
BITS_MAX = 32
CHIP_MIN, CHIP_MAX = 2, 16
SYMBOL_MAX = 65536
STRENGTH_MAX = 0.25
MAX_OFFSETS = 4096
UTTS = 64
TILE = 4096
CORR_TILE = 2048
CORR_THREADS = 128
V_SCALE, V_MAX = 64.0, 127
GOLDEN = 0x9E3779B97F4A7C15
DEFAULTS = dict(payload_bits=16, chip=8, chips_per_symbol=64, strength=0.02)   # untuned

Params = collections.namedtuple('Params', 'key payload payload_bits chip chips_per_symbol strength')
Detection = collections.namedtuple('Detection', 'offset n score energy payload T S')


def params(key, payload=0, payload_bits=16, chip=8, chips_per_symbol=64, strength=0.02):
    return Params(int(key) & (2 ** 64 - 1), int(payload) & (2 ** 32 - 1), payload_bits, chip, chips_per_symbol, float(strength))


def hash64(key, q):
    """splitmix64's finaliser of key + GOLDEN (q + 1), q an array of chip numbers"""
    with np.errstate(over='ignore'):
        z = np.uint64(key) + np.uint64(GOLDEN) * (np.asarray(q).astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def chip_sign(key, q):
    """c(q): +1 where bit 63 of the hash is 0, else -1"""
    return 1 - 2 * (hash64(key, q) >> np.uint64(63)).astype(np.int64)


def pulse(t, L):
    return np.where(np.asarray(t) < L // 2, 1, -1).astype(np.int64)


def carrier(p, positions):
    """s at the carrier positions (>= 0)"""
    pos = np.asarray(positions, np.int64)
    q = pos // p.chip
    j = (q // p.chips_per_symbol) % p.payload_bits
    bit = (np.int64(p.payload) >> j) & 1
    return chip_sign(p.key, q) * pulse(pos % p.chip, p.chip) * (1 - 2 * bit)


def blocks(n):
    return -(-n // BLOCK)


def magnitude(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), np.abs(x), np.float32(0)).astype(np.float32)


def block_max(x):
    """E[k], float32"""
    m = magnitude(x)
    E = np.zeros(blocks(len(m)), np.float32)
    for k in range(len(E)):
        E[k] = m[k * BLOCK:(k + 1) * BLOCK].max()
    return E


def envelope(x):
    """e[i] = min(E[k - 1], E[k], E[k + 1]) with 0 outside the row, float32"""
    n = len(x)
    if n == 0:
        return np.zeros(0, np.float32)
    E = np.concatenate([[np.float32(0)], block_max(x), [np.float32(0)]]).astype(np.float32)
    per_block = np.minimum(np.minimum(E[:-2], E[1:-1]), E[2:])
    return np.repeat(per_block, BLOCK)[:n]


def embed(x, p):
    """-> (out float32, marked bool): a product, a product by +-1, a sum, one rounding to float32"""
    x = np.asarray(x, np.float32)
    g = np.float64(p.strength) * envelope(x).astype(np.float64)
    marked = (g != 0) & np.isfinite(x)
    t = g * carrier(p, np.arange(len(x))).astype(np.float64)
    with np.errstate(all='ignore'):
        y = (x.astype(np.float64) + t).astype(np.float32)
    return np.where(marked, y, x).astype(np.float32), marked


def embed_stats(x, p):
    out, marked = embed(x, p)
    a = np.abs(out[~np.isnan(out)])                # (a NaN is passed over)
    return len(out), int(marked.sum()), np.float32(a.max() if len(a) else 0)


def v_of(r):
    """v, int64 in -127 .. 127"""
    r = np.asarray(r, np.float32)
    e = envelope(r).astype(np.float64)
    ok = np.isfinite(r) & (e > 0)
    with np.errstate(all='ignore'):
        z = np.rint(V_SCALE * np.where(ok, r, 0).astype(np.float64) / np.where(ok, e, 1.0))
    return np.where(ok, np.clip(z, -V_MAX, V_MAX), 0).astype(np.int64)


def chips(n, L):
    return (n + 2 * L - 2) // L


def chip_sums(v, L, f):
    """A_f[i], i < chips(n, L): the sum of v[s] m((s + f) mod L) over (s + f) // L == i"""
    n = len(v)
    A = np.zeros(chips(n, L), np.int64)
    pos = np.arange(n) + f
    np.add.at(A, pos // L, v * pulse(pos % L, L))
    return A


def _pick(n, T, S_all, energy, P):
    offset = int(np.argmax(T))                     # (the first of the largest)
    S = S_all[offset]
    payload = sum(1 << j for j in range(P) if S[j] < 0)
    return Detection(offset, n, int(T[offset]), int(energy[offset]), payload, T, S)


def detect(r, p, D):
    """the chip-sum form"""
    v = v_of(r)
    n, L, C, P = len(v), p.chip, p.chips_per_symbol, p.payload_bits
    nch = chips(n, L)
    signs = chip_sign(p.key, np.arange(nch + (D - 1) // L + 1))
    S_all = np.zeros((D, P), np.int64)
    energy = np.zeros(D, np.int64)
    for f in range(min(L, D)):
        A = chip_sums(v, L, f)
        e = int(np.sum(A * A))
        i = np.arange(nch)
        for w in range((D - 1 - f) // L + 1):
            d = w * L + f
            j = ((i + w) // C) % P
            s = np.bincount(j, weights=(signs[w:w + nch] * A).astype(np.float64), minlength=P)
            S_all[d] = s.astype(np.int64)
            energy[d] = e
    return _pick(n, np.abs(S_all).sum(axis=1), S_all, energy, P)


def detect_brute(r, p, D):
    """the definition: every offset over every sample"""
    v = v_of(r)
    n, L, C, P = len(v), p.chip, p.chips_per_symbol, p.payload_bits
    S_all = np.zeros((D, P), np.int64)
    energy = np.zeros(D, np.int64)
    for d in range(D):
        a = {}
        for i in range(n):
            q = (i + d) // L
            a[q] = a.get(q, 0) + int(v[i]) * (1 if (i + d) % L < L // 2 else -1)
        for q, aq in a.items():
            c = int(chip_sign(p.key, np.array([q]))[0])
            S_all[d, (q // C) % P] += c * aq
            energy[d] += aq * aq
    return _pick(n, np.abs(S_all).sum(axis=1), S_all, energy, P)


def zeta(score, energy, P):
    """(score - sqrt(2 P energy / pi)) / sqrt(energy (1 - 2 / pi)): under no mark S[j] is about normal with variance energy / P, so
    score is a sum of P half-normals of total variance energy; 0 where energy is 0"""
    if energy <= 0:
        return 0.0
    return (score - math.sqrt(2.0 * P * energy / math.pi)) / math.sqrt(energy * (1.0 - 2.0 / math.pi))


# ---- sizes (csrc/watermark_plan.h)
def tiles(n):
    return -(-n // TILE)


def corr_tiles(n, L):
    return -(-chips(n, L) // CORR_TILE)


def shifts(D, L):
    return (D - 1) // L + 1


def corr_shifts(D, L):
    sw = 1
    while sw < shifts(D, L) and sw < CORR_THREADS:
        sw *= 2
    return sw


def corr_ranges(D, L):
    return -(-shifts(D, L) // corr_shifts(D, L))


def sign_words(n, L, D):
    return (corr_tiles(n, L) * CORR_TILE + corr_ranges(D, L) * corr_shifts(D, L) + 31) // 32 + 2


def corr_lds(P):
    return P * CORR_THREADS * 8 + CORR_TILE * 2 + ((CORR_TILE + CORR_THREADS) // 32 + 2) * 4
