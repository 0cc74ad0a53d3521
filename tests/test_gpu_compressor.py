"""GPU: tts_compress (csrc/compressor.hip) against the numpy oracle of tests/compressor_oracle.py -- the envelope bit for bit (it
involves no transcendental function), every NaN, Inf, zero and identity position of the output bit for bit, every other output
element within 2^-24 |y| + 2^-40 |y| + 2^-150 of the oracle's double y (compressor_cases.bound: the one rounding, and the device's
log10 and pow against numpy's).

The shapes are the smallest that reach every seam: lengths either side of a segment (256 samples) and of a tile (64 segments =
16384 samples) and over two tiles, up to five ragged rows with a fill behind each, in place and apart, buffers 4, 8 and 12 bytes off
a 16-byte boundary; attack 0 and release 0, slope 0 and slope 1, knee 0 and a knee; NaN, +-Inf, -0.0 and denormal samples, and a
burst followed by silence, whose state is carried across segments and a tile."""
import ctypes

import numpy as np
import pytest

import compressor_cases as C
import compressor_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

LENGTHS = (1, 255, 256, 257, 513, 16384, 16385, 40000)
_want = {}


def want(x, p):
    """the oracle's row, computed once per input and parameter set"""
    key = (np.asarray(x, np.float32).tobytes(), tuple(p))
    if key not in _want:
        _want[key] = O.compress(x, p)
    return _want[key]


def run(engine, X, p, n_samples=None, in_place=True, out_fill=C.FILL, envelope=True, stats=False):
    """-> (the result (B, N) float32, the envelope (B, N) float64 or None[, the records]) of host rows"""
    X = np.ascontiguousarray(X, np.float32)
    d = engine.to_device(X)
    o = d if in_place else engine.to_device(np.full(X.shape, out_fill, np.float32))
    env = None
    try:
        got = engine.compress(d, C.as_engine(p), n_samples=n_samples, out=None if in_place else o, envelope=envelope, stats=stats)
        got = got if isinstance(got, tuple) else (got,)
        assert got[0] is o
        if not in_place:
            assert np.array_equal(C.bits(d.to_host()), C.bits(X))          # the input is read only
        answer = [o.to_host(), None]
        if envelope:
            env = got[1]
            answer[1] = env.to_host()
        return tuple(answer) + ((got[-1],) if stats else ())
    finally:
        d.free()
        if not in_place:
            o.free()
        if env is not None:
            env.free()


def check_row(got, env, x, p, what):
    w = want(x, p)
    n = len(x)
    assert C.same_doubles(env[:n], w.envelope), what
    ok, worst = C.held(got[:n], w)
    assert ok, what
    assert worst <= 1.0, (what, worst)
    return w


def raw(engine, p_wav, p_out, B, N, p, n_samples=None, envelope=None, stats=None):
    H = pkg('_hip')
    ns = None if n_samples is None else np.ascontiguousarray(n_samples, np.int32)
    rec = None if p is None else H.TtsCompressor(*p)
    return engine.lib.tts_compress(engine.handle, p_wav, p_out, B, N, None if ns is None else ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   None if rec is None else ctypes.addressof(rec), envelope, stats)


@pytest.mark.parametrize('name', sorted(C.SETS))
def test_every_length_is_the_oracle(engine, name):
    p = C.params(name)
    for n in LENGTHS:
        x = C.speech_like(n, amp=1.2)
        got, env = run(engine, x[None], p, in_place=n % 2 == 0)
        w = check_row(got[0], env[0], x, p, (name, n))
        if name == 'unity':
            assert np.array_equal(C.bits(got[0]), C.bits(x))                # ratio 1, make-up 0: the row's own bits
        elif n >= 255 and name != 'unity':
            assert np.sum(w.r < 0) > 0                                       # ... and the others do compress


def test_a_row_under_the_knee_is_its_own_bits(engine):
    p = C.params('soft')                                                     # T - W / 2 = -36 dB
    x = C.speech_like(16385, amp=0.01)
    assert np.abs(x).max() < 10.0 ** (-36.5 / 20.0)
    got, env = run(engine, x[None], p._replace(makeup_db=0.0))
    assert np.array_equal(C.bits(got[0]), C.bits(x)) and env[0].max() > 0


@pytest.mark.parametrize('in_place', [True, False])
def test_a_ragged_batch_leaves_what_is_behind_its_rows(engine, in_place):
    p = C.params('speech')
    N = O.TILE + 300
    rows = [C.speech_like(n, amp=1.2) for n in (1, N, 255, O.TILE, 513)]
    X, lens = C.padded(rows, N)
    got, env, stats = run(engine, X, p, n_samples=lens, in_place=in_place, out_fill=np.float32(3.5), stats=True)
    for b, r in enumerate(rows):
        w = check_row(got[b], env[b], r, p, b)
        assert np.all(got[b, len(r):] == (C.FILL if in_place else np.float32(3.5))), b
        # the record: reduced exactly and the reduction within 1e-9 dB where the levels stay clear of the knee's lower edge (checked
        # here on the CPU); max_reduction_db is a float32: the nearest one to a value within 1e-9 of the oracle's
        assert C.clear_of_the_knee(w, p), b
        n, reduced, max_red, _peak = O.stats(w)
        assert (stats['n'][b], stats['reduced'][b]) == (n, reduced), b
        assert np.float32(max_red - 1e-9) <= stats['max_reduction_db'][b] <= np.float32(max_red + 1e-9), b
        assert stats['peak_out'][b] == np.abs(got[b, :len(r)]).max(), b


def test_a_burst_then_silence_carries_its_state_over_segments_and_a_tile(engine):
    for name in ('slow', 'speech'):
        p = C.params(name)
        x = C.burst(2 * O.TILE + 700)
        got, env = run(engine, x[None], p)
        w = check_row(got[0], env[0], x, p, name)
        assert w.s[1] > 0 and w.t[2] > 0
        if name == 'slow':                                                   # the release is still falling two tiles on
            assert w.s[-1] > 0 and w.s[O.TILE_SEGS + 1] > w.s[-1] and w.envelope[-1] > 0


def test_a_rows_bits_depend_neither_on_its_batch_nor_on_what_ran_before(engine):
    """65 rows: two launches; a row alone, in another batch at another place, and behind a call with other parameters"""
    p = C.params('soft')
    lens = [300 + 7 * b for b in range(64)] + [O.TILE + 9]
    rows = [C.speech_like(n, amp=1.2) for n in lens]
    X, ns = C.padded(rows)
    got, env = run(engine, X, p, n_samples=ns)
    for b in (0, 31, 63, 64):
        check_row(got[b], env[b], rows[b], p, b)
    run(engine, X[:3], C.params('slow'), n_samples=ns[:3])                  # (leaves other states in the workspace)
    alone = {b: run(engine, rows[b][None], p) for b in (0, 63, 64)}
    three, ns3 = C.padded([rows[64], rows[0], rows[63]])
    moved, moved_env = run(engine, three, p, n_samples=ns3, in_place=False)
    for place, b in enumerate((64, 0, 63)):
        n = lens[b]
        assert np.array_equal(C.bits(got[b, :n]), C.bits(alone[b][0][0]))
        assert np.array_equal(C.bits(moved[place, :n]), C.bits(alone[b][0][0]))
        assert C.same_doubles(env[b, :n], alone[b][1][0]) and C.same_doubles(moved_env[place, :n], alone[b][1][0])


@pytest.mark.parametrize('name', ['speech', 'hard'])
def test_non_finite_negative_zero_and_denormal_samples(engine, name):
    p = C.params(name)
    for n in (257, O.TILE + 70):
        x = C.specials(n)
        got, env = run(engine, x[None], p)
        w = check_row(got[0], env[0], x, p, (name, n))
        nan, inf = np.isnan(x), np.isinf(x)
        assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(got[0][inf], x[inf])   # a NaN at its own position alone
        assert np.all(np.isfinite(w.envelope))
    x = C.denormal(700)
    p = p._replace(makeup_db=0.0)
    got, env = run(engine, x[None], p)
    check_row(got[0], env[0], x, p, name)
    assert np.array_equal(C.bits(got[0]), C.bits(x))                        # far under any threshold: -0.0 and the denormals themselves


@pytest.mark.parametrize('off_in,off_out', [(1, 1), (2, 3), (3, 0), (0, 2)])
def test_buffers_off_a_16_byte_boundary(engine, off_in, off_out):
    """the rows start 4, 8 or 12 bytes behind a 16-byte boundary, in place (equal offsets) and apart; N is odd, so every row of
    the batch has another alignment"""
    p = C.params('speech')
    B, N = 3, O.TILE + 259
    rows = [C.speech_like(n, amp=1.2) for n in (N, 258, O.TILE - 1)]
    X, lens = C.padded(rows, N)
    room = B * N + 8
    d_in = engine.to_device(np.full(room, C.FILL, np.float32))
    d_out = d_in if off_in == off_out else engine.to_device(np.full(room, C.FILL, np.float32))
    try:
        flat = np.full(room, C.FILL, np.float32)
        flat[off_in:off_in + B * N] = X.reshape(-1)
        d_in.copy_from(flat)
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        engine._check(raw(engine, d_in.data_ptr() + 4 * off_in, d_out.data_ptr() + 4 * off_out, B, N, p, n_samples=lens))
        got = d_out.to_host()
        assert np.all(got[:off_out] == C.FILL) and np.all(got[off_out + B * N:] == C.FILL)
        got = got[off_out:off_out + B * N].reshape(B, N)
        for b, r in enumerate(rows):
            w = want(r, p)
            ok, worst = C.held(got[b, :len(r)], w)
            assert ok and worst <= 1.0, (b, worst)
            assert np.all(got[b, len(r):] == C.FILL), b
    finally:
        d_in.free()
        if d_out is not d_in:
            d_out.free()


def test_the_profile_stage_and_its_launches(engine):
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        run(engine, C.speech_like(700)[None], C.params('speech'))
        ms, launches = engine.profile_get('compress')
        assert launches == 5 and ms > 0                        # A, chain A, B, chain B, C
        engine.profile_reset()
        X, ns = C.padded([C.speech_like(10 + b) for b in range(65)])
        run(engine, X, C.params('speech'), n_samples=ns, stats=True)
        assert engine.profile_get('compress')[1] == 12        # two launches of rows, with the records' sixth
    finally:
        engine.set_option('profile', 0)


def test_every_refusal_returns_its_code_and_enqueues_nothing(engine):
    H = pkg('_hip')
    p = C.params('speech')
    B, N = 2, 600
    X = np.stack([C.speech_like(N), C.speech_like(N, seed=5)])
    d, o = engine.to_device(X), engine.to_device(np.full((B, N), C.FILL, np.float32))
    a, q = d.data_ptr(), o.data_ptr()
    nan = float('nan')
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        cases = {
            'wav': raw(engine, None, q, B, N, p), 'out': raw(engine, a, None, B, N, p), 'params': raw(engine, a, q, B, N, None),
            'B': raw(engine, a, q, 0, N, p), 'N': raw(engine, a, q, B, 0, p),
            'n0': raw(engine, a, q, B, N, p, n_samples=[N, 0]), 'n+': raw(engine, a, q, B, N, p, n_samples=[N + 1, 5]),
            'T+': raw(engine, a, q, B, N, p._replace(threshold_db=0.5)), 'T-': raw(engine, a, q, B, N, p._replace(threshold_db=-80.5)),
            'Tnan': raw(engine, a, q, B, N, p._replace(threshold_db=nan)),
            's-': raw(engine, a, q, B, N, p._replace(slope=-0.01)), 's+': raw(engine, a, q, B, N, p._replace(slope=1.01)),
            'W-': raw(engine, a, q, B, N, p._replace(knee_db=-1.0)), 'W+': raw(engine, a, q, B, N, p._replace(knee_db=40.5)),
            'm-': raw(engine, a, q, B, N, p._replace(makeup_db=-24.5)), 'm+': raw(engine, a, q, B, N, p._replace(makeup_db=24.5)),
            'aA1': raw(engine, a, q, B, N, p._replace(attack_coeff=1.0)), 'aA-': raw(engine, a, q, B, N, p._replace(attack_coeff=-0.1)),
            'aR1': raw(engine, a, q, B, N, p._replace(release_coeff=1.0)), 'aRnan': raw(engine, a, q, B, N, p._replace(release_coeff=nan)),
            'align': raw(engine, a + 2, q, 1, N, p), 'align_out': raw(engine, a, q + 1, 1, N, p),
            'align_env': raw(engine, a, q, 1, N, p, envelope=q + 4),
            'overlap': raw(engine, a, a + 4, 1, N, p), 'overlap_behind': raw(engine, a + 4 * N, a + 4, 1, N, p),
        }
        assert cases == dict.fromkeys(cases, H.TTS_ERR_INVALID), cases
        assert b'overlaps' in engine.lib.tts_last_error(engine.handle)
        assert engine.profile_get('compress')[1] == 0
        assert np.array_equal(C.bits(o.to_host()), C.bits(np.full((B, N), C.FILL, np.float32))) and np.array_equal(C.bits(d.to_host()), C.bits(X))
        with pytest.raises(ValueError):
            engine.compress(d, 'speech', n_samples=[N, N + 1])
        with pytest.raises(ValueError, match='ratio'):
            engine.compress(d, (-20.0, 0.5))
        # the host-only entry points
        lib = engine.lib
        aA, aR = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert lib.tts_compressor_design(22050, 5.0, 0.0, ctypes.byref(aA), ctypes.byref(aR)) == H.TTS_OK
        assert aR.value == 0.0 and abs(aA.value - O.coefficient(5.0, 22050)) <= 2e-16
        assert lib.tts_compressor_design(7999, 5.0, 50.0, ctypes.byref(aA), ctypes.byref(aR)) == \
            lib.tts_compressor_design(22050, -1.0, 50.0, ctypes.byref(aA), ctypes.byref(aR)) == \
            lib.tts_compressor_design(22050, 5.0, 10001.0, ctypes.byref(aA), ctypes.byref(aR)) == H.TTS_ERR_UNSUPPORTED
        assert lib.tts_compressor_design(22050, 5.0, 50.0, None, ctypes.byref(aR)) == H.TTS_ERR_INVALID
        rec = H.TtsCompressor()
        for name in O.PROFILES:
            assert lib.tts_compressor_profile(name.encode(), 22050, ctypes.addressof(rec)) == H.TTS_OK
            np.testing.assert_allclose([getattr(rec, f) for f, _t in rec._fields_], O.profile(name, 22050), rtol=1e-15, atol=0)
            assert tuple(H.compressor_params(('profile', name), 22050)) == tuple(O.profile(name, 22050))
        assert lib.tts_compressor_profile(b'speech', 7000, ctypes.addressof(rec)) == H.TTS_ERR_UNSUPPORTED
        assert lib.tts_compressor_profile(b'loud', 22050, ctypes.addressof(rec)) == lib.tts_compressor_profile(b'speech', 22050, None) == H.TTS_ERR_INVALID
        # the setting refuses likewise and stays as it was
        bad = H.TtsCompressor(*p._replace(slope=2.0))
        assert lib.tts_set_compressor(engine.handle, 1, None) == lib.tts_set_compressor(engine.handle, 1, ctypes.addressof(bad)) == H.TTS_ERR_INVALID
        assert engine._compressor is None
    finally:
        engine.set_option('profile', 0)
        d.free()
        o.free()
