"""GPU: tts_shift_magnitudes against tests/shift_oracle.py at the smallest shapes that can still go wrong (shift_cases.py): B = 3,
T = 70, F = 1025 at orders 2, 33 and 64, and F = 129 and 2049 once each.  Every computed element within 2^-24 |y| + eta (|t1| + |t2|)
of the float64 oracle; every copy, zero and NaN position bit for bit.  `out` holds a NaN pattern before every call, lies inside a
guard band and one float behind an allocation's start in half of the calls; the frames behind n_frames hold NaN, which a kernel
that read them would carry into its output."""
import ctypes

import numpy as np
import pytest

import shift_cases as C
import shift_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

RUNS = [('mixed', 1025, 2), ('mixed', 1025, 33), ('mixed', 1025, 64), ('mixed', 129, 33), ('mixed', 2049, 33), ('launch_seam', 1025, 33)]
_cache = {}


def _inputs(name, F):
    case = C.LISTS[name]()
    x = C.batch(case['B'], F, case['T'])
    if name == 'mixed':
        x = C.with_specials(x)
    return case, C.poisoned(x, case['n_frames'])


def _oracle(name, F, order):
    """computed once per case and left unchanged"""
    key = (name, F, order)
    if key not in _cache:
        case, x = _inputs(name, F)
        _cache[key] = O.shift(x, case['segments'], case['n_frames'], order)
    return _cache[key]


def test_the_constants_and_the_cases(engine):
    H = pkg('_hip')
    assert engine.shift_tile() == C.TILE == H.SHIFT_TILE == 8 and engine.shift_max_segments() == O.MAX_SEGMENTS == 4096
    assert engine.shift_max_order() == O.MAX_ORDER == 256
    seg = C.mixed()['segments']
    assert {q[2] for q in seg} >= {C.TILE - 1, C.TILE, C.TILE + 1}
    assert {O.STEP_MIN, O.STEP_MAX, O.UNITY} <= {q[3] for q in seg} and {O.STEP_MIN, O.STEP_MAX, O.UNITY} <= {q[4] for q in seg}
    assert any(q[3] > O.UNITY for q in seg) and any(q[3] == O.UNITY != q[4] for q in seg) and any(q[4] == O.UNITY != q[3] for q in seg)
    assert seg[0][1] > 0 and seg[2][1] > seg[1][1] + seg[1][2] and seg[-1][1] + seg[-1][2] < C.mixed()['n_frames'][2]    # gaps
    straddle = [q[0] for q in C.launch_seam()['segments']]
    assert len(straddle) == C.PER_LAUNCH + 1 and straddle[C.PER_LAUNCH - 1] == straddle[C.PER_LAUNCH] == 1


@pytest.mark.parametrize('name,F,order', RUNS)
def test_shift_is_within_the_bound_of_the_oracle(engine, name, F, order):
    H = pkg('_hip')
    case, x = _inputs(name, F)
    nf, seg = case['n_frames'], case['segments']
    want = _oracle(name, F, order)
    if name == 'mixed':
        y, comp = want['out'], want['computed']
        assert np.isnan(y[0, :, 4]).all() and np.isnan(y[0, :, 10]).all() and comp[0, 4] and comp[0, 10]     # a NaN, an Inf: the frame is NaN
        assert np.isfinite(y[0, :, 3]).all() and np.isfinite(y[0, :, 5]).all() and np.isfinite(y[0, :, 9]).all() and np.isfinite(y[0, :, 11]).all()
        assert comp[0, 22] and not y[0, :, 22].view(np.uint32).any()                                        # an all-zero frame: +0.0
        tiny = np.abs(y[0, :, 38])
        assert comp[0, 38] and ((tiny > 0) & (tiny < 2.0 ** -126)).any()                                    # denormals come out
        assert comp[0, 37] and y[0, 10, 37] < 0 and (y[0, 16:, 37] > 0).all()                               # the sign follows x: bin 10 reads bin 5
        assert not comp[0, 30] and y.view(np.uint32)[0, 7, 30] == 0x7fc12345 and y.view(np.uint32)[0, 8, 31] == 0x80000000
    worst = 0.0
    for shift in (0, 1):
        rc, got, around = C.raw_shift(engine, H, x, nf, seg, order, shift)
        assert rc == 0, engine.lib.tts_last_error(engine.handle)
        assert (around == C.NAN_PATTERN).all()                                  # the guard band: nothing outside out[B][F][T] is written
        assert not (got == C.NAN_PATTERN).any()                                 # ... and every element of it is
        worst = max(worst, O.assert_holds(got, want, (name, F, order, shift)))
    print('shift {} F={} order={}: worst |out - y| / bound = {:.3g}'.format(name, F, order, worst))
    for b, n in enumerate(nf):
        assert not want['out'][b, :, n:].view(np.uint32).any()                  # +0.0 behind a row
    if (F, order) != (1025, 33):
        return
    # the binding: a fresh array from a device buffer and from a host array, and into a buffer of the caller's
    d = engine.to_device(x)
    mine = engine.empty(x.shape)
    try:
        assert engine.shift_plan(x.shape, seg, nf, order) == O.launches(len(seg))
        for src in (d, x):
            out = engine.shift_magnitudes(src, seg, nf, order)
            try:
                O.assert_holds(out.to_host().view(np.uint32), want, (name, 'binding'))
            finally:
                out.free()
        assert engine.shift_magnitudes(d, seg, nf, order, out=mine) is mine
        O.assert_holds(mine.to_host().view(np.uint32), want, (name, 'out='))
    finally:
        mine.free()
        d.free()


def test_a_row_alone_is_the_row_in_the_batch(engine):
    """bit for bit: rows 0 and 1 of `mixed` alone, row 1 as row 0 of a batch of two, and `launch_seam` cut into one list per row"""
    H = pkg('_hip')
    case, x = _inputs('mixed', 1025)
    nf, seg = case['n_frames'], case['segments']
    rc, whole, _a = C.raw_shift(engine, H, x, nf, seg, 33)
    assert rc == 0
    for b in (0, 1):
        own = [(0,) + q[1:] for q in seg if q[0] == b]
        rc, got, _a = C.raw_shift(engine, H, x[b:b + 1], [nf[b]], own, 33)
        assert rc == 0 and np.array_equal(got[0], whole[b]), b
    pair = [(0,) + q[1:] for q in seg if q[0] == 1] + [(1,) + q[1:] for q in seg if q[0] == 0]
    rc, got, _a = C.raw_shift(engine, H, x[[1, 0]], [nf[1], nf[0]], pair, 33)
    assert rc == 0 and np.array_equal(got[0], whole[1]) and np.array_equal(got[1], whole[0])
    other, y = _inputs('launch_seam', 1025)
    rc, both, _a = C.raw_shift(engine, H, y, other['n_frames'], other['segments'], 33)
    assert rc == 0
    for b in (0, 1):
        own = [(0,) + q[1:] for q in other['segments'] if q[0] == b]
        rc, got, _a = C.raw_shift(engine, H, y[b:b + 1], [other['n_frames'][b]], own, 33)
        assert rc == 0 and np.array_equal(got[0], both[b]), b


def test_refusals_enqueue_nothing_and_a_legal_call_counts_its_launches(engine):
    H = pkg('_hip')
    case, x = _inputs('mixed', 129)
    nf, seg = case['n_frames'], case['segments']
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(seg)]
    many = [(0, s % 70, 1, 65536, 65536) for s in range(4097)]
    cases = [
        (dict(in_place=True), 'out is mag: the stage does not work in place'),
        (dict(S=0), 'need B, T, S >= 1'),
        (dict(B=0), 'need B, T, S >= 1'),
        (dict(T=0), 'need B, T, S >= 1'),
        (dict(F=128), 'F = 128 is not 2^m + 1 with 2^m in 128 .. 2048'),
        (dict(F=65), 'F = 65 is not 2^m + 1 with 2^m in 128 .. 2048'),
        (dict(order=1), 'order = 1 is not in 2 .. 64'),
        (dict(order=65), 'order = 65 is not in 2 .. 64'),
        (dict(segments=many, B=1, n_frames=[70]), '4097 segments are more than tts_shift_max_segments() = 4096'),
        (dict(B=3, S=2), '3 rows of 2 segments: no row is without a segment'),
        (dict(n_frames=[70, 71, 9]), 'n_frames[1] = 71 is not in 1 .. T = 70'),
        (dict(n_frames=[70, 41, 0]), 'n_frames[2] = 0 is not in 1 .. T = 70'),
        (dict(segments=edit(0, 0, 1)), 'row of segment 0 is 1: the rows start at 0'),
        (dict(segments=edit(7, 0, 0)),'row of segment 8 is 2 and follows 0: the rows are non-decreasing and none is without a segment'),
        (dict(segments=seg[:-1]), 'row of segment 7 is 1: the last row is B - 1 = 2'),
        (dict(segments=edit(1, 2, 0)), 'segment 1 has 0 frames: at least 1 is needed'),
        (dict(segments=edit(7, 2, 42)), 'segment 7 covers frames 0 .. 41 of row 1, which has 0 .. 40'),
        (dict(segments=edit(0, 1, -1)), 'segment 0 covers frames -1 .. 5 of row 0, which has 0 .. 69'),
        (dict(segments=edit(1, 1, 8)), "segment 1 starts at frame 8 of row 0, in front of its predecessor's end 9: the ranges of a row ascend and do "
                                       'not overlap'),
        (dict(segments=[q[:3] + (3,) + q[3:] if s == 2 else q for s, q in enumerate(seg)]), 'segment 2 has reserved = 3, which must be 0'),
        (dict(segments=edit(4, 3, 32767)), 'segment 4 has pitch_step 32767, which is not in 32768 .. 131072'),
        (dict(segments=edit(4, 4, 131073)), 'segment 4 has formant_step 131073, which is not in 32768 .. 131072'),
    ]
    d = engine.to_device(x)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        for kw, text in cases:
            rc, got, around = C.raw_shift(engine, H, x, kw.get('n_frames', nf), kw.get('segments', seg), kw.get('order', 33), 0, kw.get('S'), kw.get('B'),
                                          kw.get('F'), kw.get('T'), kw.get('in_place', False))
            assert rc == H.TTS_ERR_INVALID, (kw, rc)
            assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'shift_magnitudes: ' + text, kw
            assert (got == C.NAN_PATTERN).all() and (around == C.NAN_PATTERN).all()
        # NULL pointers and a misaligned buffer: the library itself
        q = C.segment_array(H, seg)
        pn = np.asarray(nf, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out = engine.empty((3, 129, 70))
        try:
            null = 'a NULL pointer (mag, segments and out are required)'
            for args, text in (((None, 3, 129, 70, pn, q.ctypes.data, len(q), 33, out.data_ptr()), null),
                               ((d.data_ptr(), 3, 129, 70, pn, None, len(q), 33, out.data_ptr()), null),
                               ((d.data_ptr(), 3, 129, 70, pn, q.ctypes.data, len(q), 33, None), null),
                               ((d.data_ptr(), 3, 129, 70, pn, q.ctypes.data, len(q), 33, out.data_ptr() + 2), 'the buffers must be 4-byte aligned')):
                assert engine.lib.tts_shift_magnitudes(engine.handle, *args) == H.TTS_ERR_INVALID
                assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'shift_magnitudes: ' + text
        finally:
            out.free()
        with pytest.raises(ValueError):
            engine.shift_magnitudes(d, edit(4, 3, 32767), nf, 33)
        with pytest.raises(ValueError):
            engine.shift_magnitudes(d, seg, nf, 65)
        assert engine.profile_get('shift') == (0.0, 0)
        # legal calls: the launches the plan predicts, and no other stage moves
        engine.shift_magnitudes(d, seg, nf, 33).free()
        assert engine.profile_get('shift')[1] == O.launches(len(seg)) == 1
        other, y = _inputs('launch_seam', 129)
        engine.profile_reset()
        engine.shift_magnitudes(y, other['segments'], other['n_frames'], 33).free()
        assert engine.profile_get('shift')[1] == O.launches(len(other['segments'])) == 2
        for stage in ('warp', 'stretch', 'resample', 'denorm', 'gl_iter'):
            assert engine.profile_get(stage) == (0.0, 0), stage
    finally:
        engine.set_option('profile', 0)
        d.free()


def test_a_tone_keeps_its_formants_and_moves_its_pitch(engine):
    """The one test that listens: a 150 Hz tone of 60 hops through Engine.pitch_shift(.., preserve_formants=True) at +4 semitones,
    tracked by Engine.f0.  The ratio of the median voiced F0 to the tracker's reading of the input is held to the same figure
    computed on the CPU oracles -- shift_oracle, the Griffin-Lim of oracle/audio_oracle.py, tests/f0_oracle.py -- with the same seed
    and iterations, within 1e-3 (the tracker bound of tests/test_gpu_prosody_pitch.py): the device differs from the oracles by
    roundings only."""
    import listening_shift as L
    got = L.device_ratio(engine)
    want = L.oracle_ratio()
    print('F0 ratio at +4 semitones: device {:.6f}, oracles {:.6f}, 2 ** (4 / 12) = {:.6f}'.format(got, want, 2 ** (4 / 12)))
    assert abs(got - want) <= 1e-3
