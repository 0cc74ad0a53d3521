"""GPU: tts_warp_magnitudes against tests/warp_oracle.py, bit for bit, at the smallest shapes that can still go wrong
(warp_cases.py): F of 1, 3 and 1025, T of at most 40 (65 at the tile seam), B of 1, 3 and 65; `out` holds a NaN pattern before every
call and lies one float behind an allocation's start in half of them; the frames behind n_frames hold NaN, which a kernel that
read them would carry into its output."""
import ctypes

import numpy as np
import pytest

import warp_cases as C
import warp_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

RUNS = [('mixed', 1), ('mixed', 3), ('mixed', 1025), ('tile_seam', 3), ('launch_seam', 3), ('one_beyond_a_launch', 1)]


def _inputs(name, F):
    case = C.LISTS[name]()
    x = C.poisoned(C.with_specials(C.batch(case['B'], F, case['T'])), case['n_frames'])
    return case, x


def test_the_constants_and_the_cases(engine):
    assert engine.warp_tile() == C.TILE == 64 and engine.warp_max_segments() == O.MAX_SEGMENTS == 4096
    seg = C.mixed()['segments']
    speech = [q for q in seg if q[2] > 0]
    assert {q[4] for q in speech} >= set(C.STEPS) and {q[5] for q in speech} >= set(C.GAINS)
    assert seg[0][3] > 0 and seg[3][3] > 0 and seg[4][3] > 0 and seg[13][3] > 0 and seg[13][0] == 1            # pauses first, adjacent and last
    assert speech[0][1] > speech[1][1] and seg[2] == seg[5]                                                         # out of order, repeated
    _why, _n, counts = O.plan(C.tile_seam()['segments'], 1, 65)
    assert {C.TILE - 1, C.TILE, C.TILE + 1} <= set(counts)
    straddle = [q[0] for q in C.launch_seam()['segments']]
    assert straddle[C.PER_LAUNCH - 1] == straddle[C.PER_LAUNCH] == 1 and len(C.one_beyond_a_launch()['segments']) == C.PER_LAUNCH + 1


@pytest.mark.parametrize('name,F', RUNS)
def test_warp_is_the_oracle(engine, name, F):
    H = pkg('_hip')
    case, x = _inputs(name, F)
    B, T, nf, seg = case['B'], case['T'], case['n_frames'], case['segments']
    T_out = C.t_out_of(case)
    want, n_out = O.warp(x, seg, nf, T_out)
    if name == 'mixed':
        assert np.isnan(want).any() and np.isinf(want).any() and (want.view(np.uint32) == 0x80000000).any()
        tiny = np.abs(want[np.isfinite(want)])
        assert ((tiny > 0) & (tiny < 2.0 ** -126)).any()                                                            # a denormal survives
    for shift in (0, 1):
        rc, got, around = C.raw_warp(engine, H, x, nf, seg, T_out, shift)
        assert rc == 0, engine.lib.tts_last_error(engine.handle)
        assert (around == C.NAN_PATTERN).all()                                  # the canary: nothing outside out[B][F][T_out] is written
        assert not (got == C.NAN_PATTERN).any()                                 # ... and every element of it is
        C.assert_same(got, want, (name, F, shift))
    for b, n in enumerate(n_out):
        assert n < T_out and not want[b, :, n:].view(np.uint32).any()          # +0.0 behind a row
    # the binding: a fresh (B, F, longest) array and the plan's lengths, from a device buffer and from a host array
    d = engine.to_device(x)
    try:
        assert engine.warp_plan(x.shape, seg, nf).tolist() == n_out
        for src in (d, x):
            out, got_n = engine.warp_magnitudes(src, seg, nf)
            try:
                assert got_n.tolist() == n_out and out.shape == (B, F, max(n_out))
                C.assert_same(out.to_host().view(np.uint32), want[:, :, :max(n_out)], (name, F, 'binding'))
            finally:
                out.free()
    finally:
        d.free()


def test_nan_lands_where_the_oracle_puts_it_and_nowhere_else(engine):
    """one NaN source frame reaches the output frames that read it as i or as i + 1 -- under a == 0 too -- and no other"""
    H = pkg('_hip')
    x = C.batch(1, 3, 40)
    x[0, 1, 20] = np.nan
    seg = [(0, 10, 10, 0, 65536, 1.0),      # frames 10 .. 19: j = 9 reads 20 as i + 1 with a == 0
           (0, 0, 0, 2, 0, 0.0),
           (0, 18, 6, 0, 32768, 0.0),       # gain 0, positions 18, 18.5, .. 23.5: 19 (a == 0) and 19.5 read it as i + 1, 20 and 20.5 as i
           (0, 21, 5, 0, 65537, 1.0)]       # never reads frame 20
    want, n_out = O.warp(x, seg, None, 40)
    rc, got, _a = C.raw_warp(engine, H, x, None, seg, 40)
    assert rc == 0
    C.assert_same(got, want, 'nan')
    nan = np.isnan(got.view(np.float32))
    assert not nan[0, 0].any() and not nan[0, 2].any()
    assert np.flatnonzero(nan[0, 1]).tolist() == [9, 12 + 2, 12 + 3, 12 + 4, 12 + 5] and n_out == [29]


@pytest.mark.parametrize('q', C.CONTAINED_STEPS)
def test_the_warp_contains_the_uniform_stretch(engine, q):
    """one whole-row segment at q / 65536 with gain 1 is tts_stretch_magnitudes at that rate: the lengths and the bits, n = 1 .. 40"""
    n = list(range(1, 41))
    x = C.poisoned(C.with_specials(C.batch(40, 3, 40)), n)
    x[7, 1, 4] = np.nan                                                         # (inside row 7's 8 frames; every rate here reads frame 4)
    rate = q / 65536.0
    seg = [(b, 0, n[b], 0, q, 1.0) for b in range(40)]
    d = engine.to_device(x)
    try:
        out, n_out = engine.warp_magnitudes(d, seg, n)
        assert n_out.tolist() == [engine.stretched_frames(v, rate) for v in n]
        st = engine.stretch_magnitudes(d, rate, n)
        try:
            assert out.shape == st.shape
            a, b = out.to_host(), st.to_host()
            assert np.isnan(a).any() and np.array_equal(np.isnan(a), np.isnan(b))
            assert np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])
        finally:
            st.free()
            out.free()
    finally:
        d.free()


def test_refusals_enqueue_nothing_and_a_legal_call_counts_its_launches(engine):
    H = pkg('_hip')
    case, x = _inputs('mixed', 3)
    nf, seg = case['n_frames'], case['segments']
    T_out = C.t_out_of(case)
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(seg)]
    many = [(0, 0, 1, 0, 65536, 1.0)] * 4097
    cases = [
        (dict(S=0), 'need B, F, T, S >= 1'),
        (dict(B=0), 'need B, F, T, S >= 1'),
        (dict(segments=many, B=1, n_frames=[40]), '4097 segments are more than tts_warp_max_segments() = 4096'),
        (dict(n_frames=[40, 41, 1]), 'n_frames[1] = 41 is not in 1 .. T = 40'),
        (dict(n_frames=[40, 23, 0]), 'n_frames[2] = 0 is not in 1 .. T = 40'),
        (dict(segments=edit(0, 0, 1)), 'row of segment 0 is 1: the rows start at 0'),
        (dict(segments=edit(5, 0, 1)), 'row of segment 6 is 0 and follows 1: the rows are non-decreasing and none is without a segment'),
        (dict(segments=[q for q in seg if q[0] != 1]), 'row of segment 9 is 2 and follows 0: the rows are non-decreasing and none is without a segment'),
        (dict(segments=seg[:-1]), 'row of segment 13 is 1: the last row is B - 1 = 2'),
        (dict(segments=edit(9, 2, 19)), 'segment 9 reads frames 5 .. 23 of row 1, which has 0 .. 22'),
        (dict(segments=edit(1, 1, -1)), 'segment 1 reads frames -1 .. 18 of row 0, which has 0 .. 39'),
        (dict(segments=edit(2, 3, 4)), 'segment 2 is both speech (12 frames) and a pause (4 frames)'),
        (dict(segments=edit(0, 3, 0)), 'segment 0 is neither speech nor a pause (frames and pause are 0)'),
        (dict(segments=edit(2, 4, 16383)), 'segment 2 has step 16383, which is not in 16384 .. 262144'),
        (dict(segments=edit(2, 4, 262145)), 'segment 2 has step 262145, which is not in 16384 .. 262144'),
        (dict(segments=edit(2, 5, float('nan'))), 'segment 2 has a gain that is not finite or lies outside 0 .. 16'),
        (dict(segments=edit(2, 5, float('inf'))), 'segment 2 has a gain that is not finite or lies outside 0 .. 16'),
        (dict(segments=edit(2, 5, -0.5)), 'segment 2 has a gain that is not finite or lies outside 0 .. 16'),
        (dict(segments=edit(2, 5, 16.5)), 'segment 2 has a gain that is not finite or lies outside 0 .. 16'),
        (dict(T_out=T_out - 4), 'T_out = {} is below n_out[0] = {}'.format(T_out - 4, T_out - 3)),
    ]
    d = engine.to_device(x)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        for kw, text in cases:
            s = kw.get('segments', seg)
            rc, got, around = C.raw_warp(engine, H, x, kw.get('n_frames', nf), s, kw.get('T_out', T_out), 0, kw.get('S'), kw.get('B'))
            assert rc == H.TTS_ERR_INVALID, (kw, rc)
            assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'warp_magnitudes: ' + text, kw
            assert (got == C.NAN_PATTERN).all() and (around == C.NAN_PATTERN).all()
        # NULL pointers, F < 1 and a misaligned buffer: the library itself
        q = C.segment_array(H, seg)
        n32 = np.asarray(nf, np.int32)
        pn = n32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out = engine.empty((3, 3, T_out))
        try:
            for args, text in (((None, 3, 3, 40, pn, q.ctypes.data, len(q), T_out, out.data_ptr()), 'a NULL pointer (mag, segments and out are required)'),
                               ((d.data_ptr(), 3, 3, 40, pn, None, len(q), T_out, out.data_ptr()), 'a NULL pointer (mag, segments and out are required)'),
                               ((d.data_ptr(), 3, 3, 40, pn, q.ctypes.data, len(q), T_out, None), 'a NULL pointer (mag, segments and out are required)'),
                               ((d.data_ptr(), 3, 0, 40, pn, q.ctypes.data, len(q), T_out, out.data_ptr()), 'need B, F, T, S >= 1'),
                               ((d.data_ptr(), 3, 3, 0, pn, q.ctypes.data, len(q), T_out, out.data_ptr()), 'need B, F, T, S >= 1'),
                               ((d.data_ptr(), 3, 3, 40, pn, q.ctypes.data, len(q), T_out, out.data_ptr() + 2), 'the buffers must be 4-byte aligned')):
                assert engine.lib.tts_warp_magnitudes(engine.handle, *args) == H.TTS_ERR_INVALID
                assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'warp_magnitudes: ' + text
        finally:
            out.free()
        with pytest.raises(ValueError):
            engine.warp_magnitudes(d, edit(2, 4, 16383), nf)
        assert engine.profile_get('warp') == (0.0, 0)
        # legal calls: the launches the plan predicts, and the stretch's stage does not move
        before = engine.profile_get('stretch')
        engine.warp_magnitudes(d, seg, nf)[0].free()
        assert engine.profile_get('warp')[1] == O.launches(len(seg)) == 1
        for name in ('launch_seam', 'one_beyond_a_launch'):
            other, y = _inputs(name, 1)
            engine.profile_reset()
            engine.warp_magnitudes(y, other['segments'], other['n_frames'])[0].free()
            assert engine.profile_get('warp')[1] == O.launches(len(other['segments'])) == 2
            assert engine.profile_get('stretch') == (0.0, 0)
        assert before == (0.0, 0)
    finally:
        engine.set_option('profile', 0)
        d.free()
