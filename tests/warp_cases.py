"""Inputs of the prosody-warp tests (a plain helper module): the batches, the segment lists and how a result is held against
tests/warp_oracle.py.  A segment is a row ``(row, first, frames, pause, step, gain)``; the shapes are the smallest at which the
kernel can still go wrong -- F of 1, 3 and 1025 (fewer bins than the waves of a workgroup, and a last bin group of one), T of at
most 40 except where a tile seam needs 65 frames."""
import ctypes

import numpy as np

import segment_cases as SC
import warp_oracle as O
from segment_cases import NAN_PATTERN, poisoned   # noqa: F401 (re-exported)

TILE = O.TILE                       # tts_warp_tile(): the output frames of a segment one workgroup writes
PER_LAUNCH = O.SEGMENTS_PER_LAUNCH  # segments whose entries travel with one launch
STEPS = (16384, 65536, 65537, 262144)
GAINS = (0.0, 1.0, 0.5, 16.0)
CONTAINED_STEPS = (16384, 52429, 65536, 78643, 262144)


def batch(B, F, T):
    """(B, F, T) float32 magnitudes in the reference layout: positive, spread over six decades, with a column of exact zeros"""
    rng = np.random.default_rng([F, T, B, 19])
    x = (rng.random((B, F, T)) * np.power(10.0, rng.integers(-4, 2, (B, F, T)))).astype(np.float32)
    x[:, :, T // 2] = 0.0
    return x


def with_specials(x):
    """x with denormals (frames 0, 1, 2), a NaN (3), +Inf (5), -Inf (6) and two neighbouring -0.0 (8, 9: their blend is -0.0) in
    bin 0 of row 0 -- and 20 frames later in its last bin, where the row is that long"""
    x = x.copy()
    T = x.shape[2]
    for t, v in zip((0, 1, 2, 3, 5, 6, 8, 9), (1e-42, 1e-42, -3e-45, np.nan, np.inf, -np.inf, -0.0, -0.0)):
        if t < T:
            x[0, 0, t] = v
        if t + 20 < T:
            x[0, -1, t + 20] = v
    return x


def mixed():
    """B = 3, T = 40, ragged: a pause first, segments out of source order, a repeated one, every step and gain, adjacent pauses, a
    pause last, a row of one frame; with_specials' NaN in frame 3 of row 0 is read as i + 1 under a == 0 by the segment from frame 2"""
    n = [40, 23, 1]
    seg = [(0, 0, 0, 5, 0, 0.0),                       # a pause first (step and gain of a pause are ignored)
           (0, 20, 20, 0, 65537, 1.0),                 # out of source order: the end of the row first, up to its last frame
           (0, 0, 12, 0, 16384, 0.5),
           (0, 0, 0, 2, 65536, 1.0), (0, 0, 0, 1, 65536, 1.0),   # adjacent pauses
           (0, 0, 12, 0, 16384, 0.5),                  # repeated
           (0, 2, 7, 0, 65536, 16.0),                  # a == 0 everywhere: frames 3 .. 9 are read as i + 1 with weight 0
           (0, 7, 30, 0, 262144, 0.0),                 # gain 0: +0.0, and NaN where a NaN or Inf is read
           (0, 39, 1, 0, 65536, 1.0),                  # the row's last frame: i + 1 reads as 0.0
           (1, 5, 18, 0, 78643, 1.0),                  # up to n_frames[1] - 1: frame 23 is never fetched
           (1, 0, 0, 3, 0, 0.0),
           (1, 22, 1, 0, 16384, 2.0),
           (1, 0, 23, 0, 262144, 1.0),
           (1, 0, 0, 4, 0, 0.0),                       # a pause last
           (2, 0, 1, 0, 16384, 1.0)]                   # one frame at the slowest rate: four output frames
    return dict(B=3, T=40, n_frames=n, segments=seg)


def tile_seam():
    """B = 1, T = 65: speech and pauses of TILE - 1, TILE and TILE + 1 output frames, and one of 4 TILE + 1 at the slowest rate"""
    seg = []
    for c in (TILE - 1, TILE, TILE + 1):
        seg.append((0, 65 - c, c, 0, 65536, 1.0))
        seg.append((0, 0, 0, c, 0, 0.0))
        seg.append((0, 0, c, 0, 65537, 0.5))
    seg.append((0, 0, 65, 0, 16384, 1.0))
    return dict(B=1, T=65, n_frames=None, segments=seg)


def launch_seam():
    """B = 3, T = 40: PER_LAUNCH - 4 segments in row 0, ten in row 1 -- they straddle two launches -- and three in row 2"""
    rng = np.random.default_rng(5)
    n = [40, 40, 39]
    seg = []
    for row, k in ((0, PER_LAUNCH - 4), (1, 10), (2, 3)):
        for _ in range(k):
            if rng.random() < 0.2:
                seg.append((row, 0, 0, int(rng.integers(1, 4)), 0, 0.0))
            else:
                first = int(rng.integers(0, n[row]))
                seg.append((row, first, int(rng.integers(1, min(6, n[row] - first) + 1)), 0, int(rng.integers(O.STEP_MIN, O.STEP_MAX + 1)),
                            float(np.float32(rng.random() * 2))))
    return dict(B=3, T=40, n_frames=n, segments=seg)


def one_beyond_a_launch():
    """B = 65, T = 8: one segment per row -- a list one longer than one launch carries"""
    rng = np.random.default_rng(6)
    n = [int(v) for v in rng.integers(1, 9, 65)]
    return dict(B=65, T=8, n_frames=n, segments=[(b, 0, n[b], 0, STEPS[b % 4], GAINS[(b // 4) % 4]) for b in range(65)])


LISTS = dict(mixed=mixed, tile_seam=tile_seam, launch_seam=launch_seam, one_beyond_a_launch=one_beyond_a_launch)


def t_out_of(case, extra=3):
    why, n_out, _c = O.plan(case['segments'], case['B'], case['T'], case['n_frames'])
    assert why is None, why
    return max(n_out) + extra


def segment_array(H, segments):
    """the rows as the contiguous WARP_SEGMENT array the library reads (unchecked: refusals travel through it too)"""
    return SC.segment_array(H.WARP_SEGMENT, segments)


def raw_warp(eng, H, x, n_frames, segments, T_out, shift=0, S=None, B=None):
    """tts_warp_magnitudes through the library itself: ``x`` (B, F, T) host floats go into a buffer ``shift`` floats behind an
    allocation's start, the result into one that holds NAN_PATTERN everywhere and starts ``shift`` floats behind its own:
    ``(return code, out (B, F, T_out) as uint32 bits, the floats around it)``"""
    Bx, F, T = x.shape
    B = Bx if B is None else B
    q = segment_array(H, segments)
    total = max(B, 1) * F * max(T_out, 1)
    src = eng.to_device(np.concatenate([np.full(shift, np.nan, np.float32), x.ravel()]))
    buf = eng.to_device(np.full(total + 8, NAN_PATTERN, np.uint32))
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
    try:
        rc = eng.lib.tts_warp_magnitudes(eng.handle, src.data_ptr() + 4 * shift, B, F, T, None if nf is None else nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         q.ctypes.data, len(q) if S is None else S, int(T_out), buf.data_ptr() + 4 * shift)
        host = buf.to_host()
    finally:
        buf.free()
        src.free()
    return rc, host[shift:shift + total].reshape(max(B, 1), F, max(T_out, 1)), np.concatenate([host[:shift], host[shift + total:]])


def assert_same(got_bits, want, what):
    """bits equal, and NaN exactly where the oracle has it (a NaN's payload is the arithmetic unit's own)"""
    want = np.ascontiguousarray(want, np.float32)
    got = got_bits.view(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:5])
    same = got_bits[~nan] == want.view(np.uint32)[~nan]
    assert same.all(), (what, np.argwhere(~nan)[~same][:5])
