"""Inputs of the segment-wise resampler's tests (a plain helper module): the batch, the segment lists and how a result is held
against tests/resample_segments_oracle.py.  A segment is a row ``(row, first, samples, ratio)``.  The batch is resample_cases'
ragged one -- six rows of 5000 floats that hold 1, 2, 63, 64, 700 and 5000 samples, NaN at and behind every length --, the ratios
are resample_cases.RATIOS with 1.0 as the copy; the oracle's results are computed once per case and shared."""
import ctypes

import numpy as np

import resample_cases as RC
import resample_segments_oracle as O
import segment_cases as SC
from segment_cases import NAN_PATTERN   # noqa: F401 (re-exported)

TILE = O.TILE
PER_LAUNCH = O.SEGMENTS_PER_LAUNCH
R025, R05, DOWN4, R16K, ONE, UP3, R2, R4 = RC.RATIOS
N = RC.RAGGED_N
RAGGED = RC.RAGGED

_cache = {}


def batch():
    """resample_cases.ragged_batch() with a -0.0 and a NaN with a payload inside rows 4 and 5: a copy moves them as they are, and
    the resampled segments whose windows cover the NaN are NaN there and nowhere else"""
    x = RC.ragged_batch()
    bits = x.view(np.uint32)
    bits[4, 120] = 0x80000000
    bits[4, 121] = 0x7fc12345
    bits[5, 4500] = 0x80000000
    bits[5, 4501] = 0xffc00001
    return x


def mixed():
    """B = 6: counts of 0, 1, 255, 256, 257 and several tiles; copies; segments out of source order and repeated; every ratio; a
    border inside a tile's window (row 4's neighbours at 0.5 overlap in source and their windows reach over each other's ends);
    segments at both ends of a row, whose wings the row cuts"""
    seg = [(0, 0, 1, ONE), (0, 0, 1, R025), (0, 0, 1, R2),                       # a copy, a count of 0, a count of 2 from one sample
           (1, 0, 2, R05), (1, 1, 1, R4), (1, 0, 1, R05),                        # a count of 1; the last one produces nothing
           (2, 0, 63, DOWN4), (2, 10, 20, ONE), (2, 62, 1, UP3),
           (3, 0, 64, R4), (3, 0, 64, R16K), (3, 32, 32, R025),                  # 256 = one tile exactly
           (4, 100, 255, ONE),                                                   # a copy of 255: the -0.0 and the payload NaN travel
           (4, 188, 512, R05), (4, 186, 514, R05), (4, 130, 510, R05),           # 256, 257 and 255
           (4, 355, 255, UP3), (4, 300, 1, R025), (4, 122, 578, R16K), (4, 100, 30, ONE),
           (5, 2500, 2000, R025),                                                # out of source order
           (5, 0, 2500, R2), (5, 0, 2500, R2),                                   # several tiles, repeated
           (5, 1000, 3000, DOWN4), (5, 4400, 600, ONE), (5, 0, 4400, R16K), (5, 4390, 10, R4), (5, 4000, 257, ONE)]
    return dict(B=6, n_samples=list(RAGGED), segments=seg)


def _random(rng, row, n, k):
    out = []
    for _ in range(k):
        first = int(rng.integers(0, n))
        out.append((row, first, int(rng.integers(1, min(300, n - first) + 1)), [R05, DOWN4, ONE, ONE, UP3, R2][int(rng.integers(0, 6))]))
    return out


def seam65():
    """B = 1: 65 segments in one row of 700 samples -- a launch seam inside a row"""
    return dict(B=1, n_samples=[700], rows=[4], segments=_random(np.random.default_rng(65), 0, 700, 65))


def seam130():
    """B = 3: 64 segments in row 0, 40 in row 1 and 26 in row 2 -- a launch seam between two rows and one inside a row"""
    rng = np.random.default_rng(130)
    return dict(B=3, n_samples=[700, 63, 5000], rows=[4, 2, 5],
                segments=_random(rng, 0, 700, 64) + _random(rng, 1, 63, 40) + _random(rng, 2, 5000, 26))


def ratios16():
    """B = 1: exactly 16 distinct ratios below 1 -- the quarter semitones up to four -- one of them twice, and one above 1"""
    ratios = [2.0 ** (-(k + 1) / 48.0) for k in range(16)]
    return dict(B=1, n_samples=[700], rows=[4], segments=[(0, 37 * k, 100, r) for k, r in enumerate(ratios)] + [(0, 0, 50, ratios[3]), (0, 0, 50, UP3)])


LISTS = dict(mixed=mixed, seam65=seam65, seam130=seam130, ratios16=ratios16)


def inputs(name):
    """``(case, x)``: the list and its batch -- the rows the case names (all six unless it names some) of ``batch()``"""
    case = LISTS[name]()
    x = batch()
    if 'rows' in case:
        x = np.ascontiguousarray(x[case['rows']])
    for b, n in enumerate(case['n_samples']):
        assert np.isnan(x[b, n:]).all()
    return case, x


def oracle(name, extra=0):
    """the oracle's dict of a named list at N_out = the longest row + extra (at least 1); computed once"""
    key = (name, extra)
    if key not in _cache:
        case, x = inputs(name)
        why, n_out, _c = O.plan(case['segments'], case['B'], N, case['n_samples'])
        assert why is None, why
        _cache[key] = O.resample_segments(x, case['segments'], case['n_samples'], max(max(n_out), 1) + extra)
    return _cache[key]


def segment_array(H, segments):
    """the rows as the contiguous RESAMPLE_SEGMENT array the library reads (unchecked: refusals travel through it too); a row of
    five has ``reserved`` last"""
    return SC.segment_array(H.RESAMPLE_SEGMENT, [(r[0], r[1], r[2], r[4], r[3]) if len(r) > 4 else r for r in segments])


def raw_call(eng, H, x, n_samples, segments, N_out, shift=0, S=None, B=None, want_n=True):
    """tts_resample_segments through the library itself: ``x`` (B, n) host floats go into a buffer ``shift`` floats behind an
    allocation's start, the result into one that holds NAN_PATTERN everywhere and starts ``shift`` floats behind its own:
    ``(return code, out (B, N_out) as uint32 bits, the floats around it, n_out int32 (B,))``"""
    Bx, n = x.shape
    B = Bx if B is None else B
    q = segment_array(H, segments)
    total = max(B, 1) * max(N_out, 1)
    src = eng.to_device(np.concatenate([np.full(shift, np.nan, np.float32), x.ravel()]))
    buf = eng.to_device(np.full(total + 8, NAN_PATTERN, np.uint32))
    ns = None if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32)
    got_n = np.full(max(B, 1), -7, np.int32)
    p32 = ctypes.POINTER(ctypes.c_int32)
    try:
        rc = eng.lib.tts_resample_segments(eng.handle, src.data_ptr() + 4 * shift, B, n, None if ns is None else ns.ctypes.data_as(p32), q.ctypes.data,
                                           len(q) if S is None else S, int(N_out), buf.data_ptr() + 4 * shift, got_n.ctypes.data_as(p32) if want_n else None)
        host = buf.to_host()
    finally:
        buf.free()
        src.free()
    return rc, host[shift:shift + total].reshape(max(B, 1), max(N_out, 1)), np.concatenate([host[:shift], host[shift + total:]]), got_n


def assert_matches(got_bits, want, what, R):
    """every copy and every zero bit for bit, every resampled element within resample_oracle.bound of the oracle's float64 -- and
    NaN exactly where the oracle has it"""
    got = got_bits.view(np.float32)
    assert got.shape == want['y'].shape, (what, got.shape, want['y'].shape)
    exact = want['kind'] != O.RESAMPLED
    assert np.array_equal(got_bits[exact], want['bits'][exact]), (what, np.argwhere(exact & (got_bits != want['bits']))[:5])
    res = ~exact
    nan = np.isnan(want['y']) & res
    assert np.array_equal(np.isnan(got) & res, nan), (what, np.argwhere((np.isnan(got) & res) != nan)[:5])
    ok = res & ~nan
    err = np.abs(got[ok].astype(np.float64) - want['y'][ok])
    lim = R.bound(want['y'][ok], want['sabs'][ok])
    assert (err <= lim).all(), (what, np.argwhere(ok)[err > lim][:5], float((err / np.maximum(lim, 1e-300)).max()))
