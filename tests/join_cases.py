"""Inputs of the join tests (a plain helper module): the batch, the edit lists and how a result is held against
tests/join_oracle.py.  B = 5 rows of N = 2003 samples; the lists use row 1 twice, row 3 never, and the rows out of order."""
import ctypes

import numpy as np

import join_oracle as O

B, N = 5, 2003
TILE = 512                    # tts_join_tile(): the output samples one workgroup writes
FADES = (0, 1, 7, 64)
LARGE_GAP = 700
NAN_PATTERN = 0x7fc0beef      # what `out` holds before every call: a NaN no computation makes


def batch():
    rng = np.random.default_rng(3)
    return ((rng.random((B, N)) - 0.5) * 1.8).astype(np.float32)


def pieces_of(fade, G):
    """``(pieces, groups)``: counts 1, 2, 3, 2 fade - 1, 2 fade, 2 fade + 1 and one of 3 * TILE + 1 samples, odd firsts, gaps of
    -min(f_p, f_p+1), -1, 0, 1 and LARGE_GAP in turn; G = 3 has a group of one piece in the middle."""
    counts = [3 * TILE + 1, 1, 2, 3] + [c for c in (2 * fade - 1, 2 * fade, 2 * fade + 1) if c >= 1] + [200, 2 * fade + 1, 131, 2 * fade + 6, 77, 3]
    rows = [4, 1, 0, 2, 1, 0, 4, 2, 1, 0, 4, 2, 0]
    pieces = []
    for p, c in enumerate(counts):
        first = 2 * ((37 * p) % ((N - c) // 2 + 1)) + 1 if c < N - 1 else 1
        first = min(first, N - c)
        pieces.append([rows[p % len(rows)], first, c, 0])
    P = len(pieces)
    groups = [0] * P if G == 1 else [0 if p < 4 else 1 if p == 4 else 2 for p in range(P)]
    f = O.fades(counts, fade)
    kinds = ['full', 'one', 'zero', 'plus', 'large']
    for p in range(P - 1):
        room = min(f[p], f[p + 1])
        kind = kinds[p % len(kinds)]
        pieces[p][3] = {'full': -room, 'one': -min(room, 1), 'zero': 0, 'plus': 1, 'large': LARGE_GAP}[kind]
    pieces[P - 1][3] = -12345       # (the gap of a group's last piece is ignored)
    return [tuple(q) for q in pieces], groups


def with_specials(wav, pieces):
    """the batch with a NaN, +Inf, -Inf or -0.0 at the first, the middle and the last sample of every piece of 3 samples or more,
    in turn: in the head fade (or the overlap), in the inside, and in the tail fade (or the overlap)"""
    wav = wav.copy()
    specials = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0)]
    k = 0
    for row, first, count, _gap in pieces:
        if count < 3:
            continue
        for at in (first, first + count // 2, first + count - 1):
            wav[row, at] = specials[k % 4]
            k += 1
    return wav


def n_out_of(pieces, groups, fade):
    return O.plan(pieces, groups, fade)[1]


def odd_n_out(pieces, groups, fade):
    """an N_out above the longest group that is no multiple of 4"""
    n = max(n_out_of(pieces, groups, fade)) + 2
    return n + 1 if n % 4 == 0 else n


def raw_join(eng, d_wav, shape, pieces, groups, fade, N_out, shift=0):
    """tts_join through the library itself, into a buffer that holds NAN_PATTERN everywhere and starts ``shift`` floats behind an
    allocation's start: ``(return code, out (G, N_out) as uint32 bits, the floats around it)``"""
    q = np.ascontiguousarray(pieces, dtype=np.int32).reshape(-1, 4)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    G = int(g[-1]) + 1
    total = G * N_out
    buf = eng.to_device(np.full(total + 8, NAN_PATTERN, np.uint32))
    try:
        rc = eng.lib.tts_join(eng.handle, d_wav.data_ptr(), shape[0], shape[1], q.ctypes.data, len(q), g.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), G,
                              int(fade), int(N_out), buf.data_ptr() + 4 * shift)
        host = buf.to_host()
    finally:
        buf.free()
    return rc, host[shift:shift + total].reshape(G, N_out), np.concatenate([host[:shift], host[shift + total:]])


def assert_same(got_bits, want, what):
    """bits equal, and NaN exactly where the oracle has it (a NaN's payload is the arithmetic unit's own)"""
    want = np.ascontiguousarray(want, np.float32)
    got = got_bits.view(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:5])
    same = got_bits[~nan] == want.view(np.uint32)[~nan]
    assert same.all(), (what, np.argwhere(~nan)[~same][:5])
