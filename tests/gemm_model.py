"""Host model of the bf16-split GEMM of csrc/gemm_f32.hip (a plain helper module, imported like parity.py).

What the kernel documents, restated in numpy:

  * every f32 operand is split EXACTLY into three bf16 terms, x = hi + mid + lo: truncate to the top 16 bits, subtract
    in float32, twice (`split3`);
  * a 16-deep k step is six bf16 MFMAs into one f32 accumulator, in the order hi*lo, lo*hi, mid*mid, hi*mid, mid*hi,
    hi*hi (`PAIRS`: indices into (hi, mid, lo) of A and of W).  A product of two bf16 has 16 significand bits, so a
    16-term sum of them is taken as exact (float64) and the accumulator is rounded to float32 once per MFMA;
  * the k order of the tiles (`k_order`): channel chunk outer, tap inner when `ktaps > 1 and Cin % 32 == 0` ON THE FAST
    PATHS of the loader (up to 16 taps; with the max-pool loader up to 3), linear -- k = tap * Cin + channel -- on the
    per-thread path and on the general path (more than 16 taps, pooled convolutions with Cin % 32 != 0 or more than
    3 taps).  Tiles are 32 deep, the last one zero-filled past K;
  * split-K (`splitk_slices`: 8 slices from K >= 4096): slice i covers the tiles [k_tiles * i // 8, k_tiles * (i + 1) // 8),
    each from a zero accumulator, and the partials are added in slice order in float32.

`pairs=` lets a test build the model of a kernel that has LOST one of its six products: the host tests show that such a
model lies far outside the bound the GPU tests hold the kernel to.

The float64 reference is an explicit im2col of TF 'SAME' conv1d (padl = (ktaps - 1) // 2) behind max-pool(2, 1, SAME);
beside the product it returns D[m][n] = sum_k |a'_mk| |w_nk| (a': the pooled, masked operand), the scale one f32 rounding
of a product is measured against: phi = max_mn |got - ref| / D_mn, in units of u = 2^-24."""
import numpy as np

U = 2.0 ** -24
BK = 32
STEP = 16
# (split of A, split of W) per MFMA, in the kernel's order; 0 = hi, 1 = mid, 2 = lo
PAIRS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
PAIR_NAMES = ('hi*lo', 'lo*hi', 'mid*mid', 'hi*mid', 'mid*hi', 'hi*hi')


def _trunc16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """(hi, mid, lo) float32 arrays, each a bf16 value (low 16 bits clear), hi + mid + lo == x."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        hi = _trunc16(x)
        r1 = x - hi
        mid = _trunc16(r1)
        r2 = r1 - mid
        lo = _trunc16(r2)
    return hi, mid, lo


def splitk_slices(K):
    return 8 if K >= 4096 else 1


def loader_path(Cin, ktaps, pool):
    """'uniform' (one tap per tile, tap-inner order for a convolution), 'per_thread' (linear order, tiles straddle taps)
    or 'general' (linear order, tap by division) -- the three forms of the kernel's load_tile."""
    tap_inner = ktaps > 1 and Cin % BK == 0
    uniform = ktaps == 1 or tap_inner
    fast = (uniform and ktaps <= 3) if pool else ktaps <= 16
    if not fast:
        return 'general'
    return 'uniform' if uniform else 'per_thread'


def k_order(Cin, ktaps, pool=0):
    """k index (tap * Cin + channel) at every position of the kernel's k loop, -1 where a tile is zero-filled: an int
    array of k_tiles * 32 entries."""
    K = Cin * ktaps
    k_tiles = -(-K // BK)
    if ktaps > 1 and Cin % BK == 0 and loader_path(Cin, ktaps, pool) == 'uniform':
        it = np.arange(k_tiles)
        base = (it % ktaps) * Cin + (it // ktaps) * BK
        return (base[:, None] + np.arange(BK)[None, :]).reshape(-1)
    pos = np.arange(k_tiles * BK)
    return np.where(pos < K, pos, -1)


def slice_tiles(K):
    """[(first tile, one past the last)] of every split-K slice (one slice below the threshold)."""
    k_tiles = -(-K // BK)
    s = splitk_slices(K)
    return [(k_tiles * i // s, k_tiles * (i + 1) // s) for i in range(s)]


def im2col(x, ktaps, T, pool):
    """x [M][Cin] float32, M = B * T -> a' [M][ktaps * Cin] float32: max-pool(2, 1, SAME) along each sequence, then the
    taps of TF 'SAME' conv1d with zeros outside the sequence.  Exact (a maximum and copies)."""
    x = np.asarray(x, dtype=np.float32)
    M, Cin = x.shape
    xs = x.reshape(M // T, T, Cin)
    if pool:
        xs = np.maximum(xs, np.concatenate([xs[:, 1:], xs[:, -1:]], 1))
    padl = (ktaps - 1) // 2
    xp = np.pad(xs, ((0, 0), (padl, ktaps - 1 - padl), (0, 0)))
    return np.concatenate([xp[:, j:j + T] for j in range(ktaps)], -1).reshape(M, ktaps * Cin)


def reference(x, w, ktaps, T, pool):
    """(ref, D): the float64 product of the im2col operand with w [N][ktaps * Cin], and D = |a'| |w|^T."""
    a = im2col(x, ktaps, T, pool).astype(np.float64)
    w64 = np.asarray(w, dtype=np.float64)
    return a @ w64.T, np.abs(a) @ np.abs(w64).T


def phi(got, ref, D):
    """max |got - ref| / D in units of u; where D = 0 the output must be 0 exactly (inf otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    zero = D == 0
    if np.any(got[zero] != 0):
        return float('inf')
    if zero.all():
        return 0.0
    return float(np.max(err[~zero] / D[~zero]) / U)


def model_products(a, w, order, slices, pair_sets):
    """The kernel's arithmetic on the im2col operand a [M][K] and w [N][K] (float32), for several sets of products at
    once (the six per-step products are computed once): a list of float32 [M][N] results, one per entry of pair_sets."""
    a = np.asarray(a, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    M, N = a.shape[0], w.shape[0]
    sel = np.where(order >= 0, order, 0)
    live = (order >= 0)[None, :]
    ap = np.where(live, a[:, sel], np.float32(0))
    wp = np.where(live, w[:, sel], np.float32(0))
    a3 = [t.astype(np.float64) for t in split3(ap)]
    w3 = [np.ascontiguousarray(t.astype(np.float64).T) for t in split3(wp)]
    wanted = sorted({p for ps in pair_sets for p in ps})
    outs = [None] * len(pair_sets)
    for t0, t1 in slices:
        accs = [np.zeros((M, N), np.float32) for _ in pair_sets]
        for s0 in range(t0 * BK, t1 * BK, STEP):
            prod = {(sa, sb): a3[sa][:, s0:s0 + STEP] @ w3[sb][s0:s0 + STEP] for sa, sb in wanted}
            for i, ps in enumerate(pair_sets):
                acc = accs[i]
                for p in ps:
                    acc = (acc.astype(np.float64) + prod[p]).astype(np.float32)
                accs[i] = acc
        for i, acc in enumerate(accs):
            outs[i] = acc if outs[i] is None else (outs[i] + acc).astype(np.float32)
    return outs


def model_conv_many(x, w, ktaps, T, pool, pair_sets):
    Cin = np.asarray(x).shape[1]
    return model_products(im2col(x, ktaps, T, pool), w, k_order(Cin, ktaps, pool), slice_tiles(Cin * ktaps), pair_sets)


def model_conv(x, w, ktaps, T, pool, pairs=PAIRS):
    """What tts_debug_gemm computes, by the documented arithmetic: float32 [M][N]."""
    return model_conv_many(x, w, ktaps, T, pool, [tuple(pairs)])[0]


def dropped(i):
    """PAIRS without its i-th product."""
    return tuple(p for j, p in enumerate(PAIRS) if j != i)


ALL_MODELS = [PAIRS] + [dropped(i) for i in range(len(PAIRS))]


# ---------------------------------------------------------------------------------- stages: GEMM + epilogue, CBHG tail
def weight_rows(kernel):
    """A TF kernel -- conv (k, in, out) or dense (in, out) -- as the kernel's Wt [N][K], k = tap * in + channel."""
    k = np.asarray(kernel, dtype=np.float32)
    return np.ascontiguousarray(k.reshape(-1, k.shape[-1]).T)


def dense_model_many(a, w, pair_sets):
    """The arithmetic of a dense layer (gemm_f32.hip with one tap, cbhg_tail.hip: linear k order, K zero-filled to a multiple
    of 32, no split-K below K = 4096) on a [M][K], w [N][K]."""
    K = a.shape[1]
    return model_products(a, w, k_order(K, 1), slice_tiles(K), pair_sets)


def _sigmoid32(t):
    one = np.float32(1)
    return (one / (one + np.exp(-t, dtype=np.float32))).astype(np.float32)


def highway_epilogue32(acc_h, acc_t, bh, bt, x):
    """out = relu(h) t + x (1 - t), t = sigmoid(.), in float32 as the kernels' epilogues write it"""
    one = np.float32(1)
    hh = np.maximum(acc_h + bh.astype(np.float32), np.float32(0))
    tt = _sigmoid32(acc_t + bt.astype(np.float32))
    return (hh * tt + x * (one - tt)).astype(np.float32)


def tail_chain64(p2, lifter, layers):
    """float64: relu(p2 W + b), then every highway layer; lifter = (Wt [U][c_in], b), layers = [(Wh, bh, Wt, bt)] with
    [U][U] weight rows."""
    f = np.float64
    x = np.maximum(p2.astype(f) @ lifter[0].astype(f).T + lifter[1].astype(f), 0.0)
    for wh, bh, wt, bt in layers:
        h = np.maximum(x @ wh.astype(f).T + bh.astype(f), 0.0)
        t = 1.0 / (1.0 + np.exp(-(x @ wt.astype(f).T + bt.astype(f))))
        x = h * t + x * (1.0 - t)
    return x


def tail_chain_model(p2, lifter, layers, lost=None):
    """The host chain: the model GEMM per stage with a float32 numpy epilogue.  lost = (stage, i): stage `stage` (0 = the
    lifter, l = highway layer l) runs without the i-th of its six products."""
    def pairs(stage):
        return dropped(lost[1]) if lost is not None and lost[0] == stage else PAIRS
    x = np.asarray(p2, dtype=np.float32)
    acc = dense_model_many(x, lifter[0], [pairs(0)])[0]
    x = np.maximum(acc + lifter[1].astype(np.float32), np.float32(0))
    for l, (wh, bh, wt, bt) in enumerate(layers):
        acc_h, = dense_model_many(x, wh, [pairs(l + 1)])
        acc_t, = dense_model_many(x, wt, [pairs(l + 1)])
        x = highway_epilogue32(acc_h, acc_t, bh, bt, x)
    return x
