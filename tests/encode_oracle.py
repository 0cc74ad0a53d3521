"""The delivery encoder in numpy, operation by operation as include/sstts_hip.h states it: what tts_encode (csrc/encode.hip) and
the per-sample function of csrc/encode_plan.h are held to bit for bit.  No library, no GPU.

    v = float64(x) * Q                       Q = 128 (pcm8), 32768 (pcm16, mulaw, alaw): exact
    d = 0, or the TPDF dither of (seed, b, i)
    q = rint(v + d)                          ties to even; NaN -> 0 (counted), outside [-Q, Q - 1] -> saturated (counted)
    code                                     pcm16: q, pcm8: q + 128, mulaw / alaw: ITU-T G.711 from the 16-bit q (g711.c)
"""
import numpy as np

F32, S16, U8, MULAW, ALAW = range(5)
FORMATS = (S16, U8, MULAW, ALAW)
NAMES = {S16: 'pcm16', U8: 'pcm8', MULAW: 'mulaw', ALAW: 'alaw'}
NONE, TPDF = 0, 1
WIDTH = {F32: 4, S16: 2, U8: 1, MULAW: 1, ALAW: 1}
DTYPE = {S16: np.int16, U8: np.uint8, MULAW: np.uint8, ALAW: np.uint8}
SILENCE = {S16: 0, U8: 0x80, MULAW: 0xFF, ALAW: 0xD5}
RECORD = np.dtype([('clipped', np.int32), ('nans', np.int32), ('peak', np.int32), ('n', np.int32)])

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def scale(fmt):
    return 128 if fmt == U8 else 32768


def dither(seed, b, i):
    """d of row ``b`` at the sample indices ``i`` (any integer array): float64, exact, in (-1, 1)"""
    i = np.asarray(i).astype(np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(seed % (1 << 64)) + GOLDEN * (((np.uint64(b) << np.uint64(32)) | i) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    hi = (z >> np.uint64(32)).astype(np.float64)
    lo = (z & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return (hi - lo) * 2.0 ** -32


def _segment(v, ends):
    """g711.c's search: the first index whose table entry is >= v, len(ends) if none"""
    return np.searchsorted(np.asarray(ends), v, side='left')


def lin2ulaw(q):
    """g711.c linear2ulaw on 16-bit values (audioop.lin2ulaw(., 2)): uint8"""
    v = np.asarray(q).astype(np.int64) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8159) + 33
    seg = _segment(v, [0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])
    u = np.where(seg >= 8, 0x7F, (seg << 4) | ((v >> (np.minimum(seg, 7) + 1)) & 0xF))
    return (u ^ mask).astype(np.uint8)


def lin2alaw(q):
    """g711.c linear2alaw on 16-bit values (audioop.lin2alaw(., 2)): uint8"""
    v = np.asarray(q).astype(np.int64) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    v = np.where(v >= 0, v, -v - 1)
    seg = _segment(v, [0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF])
    s = np.minimum(seg, 7)
    a = np.where(seg >= 8, 0x7F, (s << 4) | ((v >> np.where(s < 2, 1, s)) & 0xF))
    return (a ^ mask).astype(np.uint8)


def ulaw2lin(codes):
    """g711.c ulaw2linear: int16"""
    u = ~np.asarray(codes).astype(np.int64) & 0xFF
    t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(codes):
    """g711.c alaw2linear: int16"""
    a = np.asarray(codes).astype(np.int64) ^ 0x55
    t = (a & 0xF) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


ULAW_TABLE = ulaw2lin(np.arange(256))
ALAW_TABLE = alaw2lin(np.arange(256))


def code(fmt, q):
    q = np.asarray(q).astype(np.int64)
    if fmt == S16:
        return q.astype(np.int16)
    if fmt == U8:
        return (q + 128).astype(np.uint8)
    return lin2ulaw(q) if fmt == MULAW else lin2alaw(q)


def decode(fmt, codes):
    """the value a decoder makes of the codes, as float64 in [-1, 1)"""
    c = np.asarray(codes)
    if fmt == S16:
        return c.astype(np.float64) / 32768.0
    if fmt == U8:
        return (c.astype(np.float64) - 128.0) / 128.0
    return (ULAW_TABLE if fmt == MULAW else ALAW_TABLE)[c].astype(np.float64) / 32768.0


def quantise(x, fmt, d=0.0):
    """-> (q int64, clipped mask, nan mask) of float32 samples ``x`` and their dither ``d``"""
    Q = scale(fmt)
    v = np.asarray(x, np.float32).astype(np.float64) * np.float64(Q)
    with np.errstate(invalid='ignore'):
        r = np.rint(v + d)
        nan = np.isnan(r)
        clipped = ~nan & ((r < -Q) | (r > Q - 1))
    q = np.where(nan, 0.0, np.clip(r, -Q, Q - 1)).astype(np.int64)
    return q, clipped, nan


def encode_row(x, fmt, dither_mode=NONE, seed=0, b=0, n=None):
    """-> (codes of the whole row, (clipped, nans, peak, n)): samples at or behind ``n`` are the format's silence"""
    x = np.asarray(x, np.float32)
    n = len(x) if n is None else int(n)
    out = np.full(len(x), SILENCE[fmt], DTYPE[fmt])
    d = dither(seed, b, np.arange(n)) if dither_mode == TPDF else 0.0
    q, clipped, nan = quantise(x[:n], fmt, d)
    out[:n] = code(fmt, q)
    return out, (int(clipped.sum()), int(nan.sum()), int(np.abs(q).max()) if n else 0, n)


def encode(x, fmt, dither_mode=NONE, seed=0, n_samples=None):
    """a batch (B, N) -> (codes (B, N), records (B,) of RECORD)"""
    x = np.asarray(x, np.float32)
    B, N = x.shape
    out = np.empty((B, N), DTYPE[fmt])
    st = np.zeros(B, RECORD)
    for b in range(B):
        out[b], rec = encode_row(x[b], fmt, dither_mode, seed, b, None if n_samples is None else n_samples[b])
        st[b] = rec
    return out, st
