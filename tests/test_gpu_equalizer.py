"""GPU: tts_equalize (csrc/equalizer.hip) against the numpy oracle of tests/equalizer_oracle.py, bit for bit on every finite output,
NaN where the oracle has NaN.

The shapes are the smallest at which the kernels can go wrong: lengths either side of a segment (256 samples) and of a tile (64
segments = 16384 samples) and over two tiles, 1, 2, 5 and 8 sections, one row, three and 65 (two launches), ragged lengths with a
fill behind every row, in place and out of place, buffers 4, 8 and 12 bytes off a 16-byte boundary, and NaN, +-Inf, -0.0 and
denormal samples."""
import ctypes

import numpy as np
import pytest

import equalizer_cases as C
import equalizer_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 255, 256, 257, 16383, 16384, 16385, 40000)
_want = {}


def want(x, sos):
    """the oracle's row, computed once per input and cascade"""
    key = (np.asarray(x, np.float32).tobytes(), np.asarray(sos, np.float64).tobytes())
    if key not in _want:
        _want[key] = O.equalize(x, sos)
    return _want[key]


def run(engine, X, sos, n_samples=None, in_place=True, out_fill=C.FILL):
    """-> the result (B, N) float32 host of host rows"""
    X = np.ascontiguousarray(X, np.float32)
    d = engine.to_device(X)
    o = d if in_place else engine.to_device(np.full(X.shape, out_fill, np.float32))
    try:
        assert engine.equalize(d, sos, n_samples=n_samples, out=None if in_place else o) is o
        if not in_place:
            assert np.array_equal(C.bits(d.to_host()), C.bits(X))          # the input is read only
        return o.to_host()
    finally:
        d.free()
        if not in_place:
            o.free()


def raw(engine, p_wav, p_out, B, N, sos, S=None, n_samples=None):
    sos = None if sos is None else np.ascontiguousarray(sos, np.float64)
    ns = None if n_samples is None else np.ascontiguousarray(n_samples, np.int32)
    return engine.lib.tts_equalize(engine.handle, p_wav, p_out, B, N, None if ns is None else ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   None if sos is None else sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   (0 if sos is None else len(sos)) if S is None else S)


# ---- exact cases that need no oracle
@pytest.mark.parametrize('p', [250, O.TILE - 1])
def test_delays_and_a_decay_are_exact(engine, p):
    """impulses in front of a segment's seam (sample 250: the decay crosses it at k = 6) and at a tile's last sample"""
    n = O.TILE + 1500
    x = np.zeros(n, np.float32)
    x[[p, p + 3]] = (1.0, -0.625)
    one = run(engine, x[None], [[0.0, 1.0, 0.0, 0.0, 0.0]])[0]
    assert np.array_equal(one[1:], x[:-1]) and one[0] == 0                   # b = (0, 1, 0): one sample late
    eight = run(engine, x[None], [[0.0, 0.0, 0.5, 0.0, 0.0]] * 8, in_place=False)[0]
    assert np.array_equal(eight[16:], x[:-16] * np.float32(2.0 ** -8)) and not eight[:16].any()
    x[p + 3] = 0
    decay = run(engine, x[None], [[1.0, 0.0, 0.0, -0.5, 0.0]])[0]           # y[i] = x[i] + y[i - 1] / 2: 2 ** -k behind the impulse
    k = np.arange(n - p, dtype=np.float64)
    assert not decay[:p].any() and np.array_equal(decay[p:], (2.0 ** -k).astype(np.float32))
    assert decay[p + 6] == 2.0 ** -6 and decay[p + 149] > 0 and decay[p + 150] == 0


# ---- against the oracle
@pytest.mark.parametrize('S', [1, 2, 5, 8])
def test_every_length_is_the_oracle_bit_for_bit(engine, S):
    sos = C.cascade(S)
    for n in LENGTHS:
        x = C.speech_like(n)
        got = run(engine, x[None], sos, in_place=n % 2 == 0)[0]
        assert C.same(got, want(x, sos)), (n, S)
        assert np.all(np.isfinite(got)) and (n < 300 or np.abs(got).max() > 1e-3)


@pytest.mark.parametrize('in_place', [True, False])
def test_a_ragged_batch_leaves_what_is_behind_its_rows(engine, in_place):
    sos = C.cascade(5)
    N = O.TILE + 300
    rows = [C.speech_like(n) for n in (1, N, 255, O.TILE, 257, O.TILE + 1, 2)]
    X, lens = C.padded(rows, N)
    got = run(engine, X, sos, n_samples=lens, in_place=in_place, out_fill=np.float32(3.5))
    for b, r in enumerate(rows):
        assert C.same(got[b, :len(r)], want(r, sos)), b
        assert np.all(got[b, len(r):] == (C.FILL if in_place else np.float32(3.5))), b


def test_more_rows_than_a_launch_takes_and_a_row_is_its_own_bits_anywhere(engine):
    """65 rows: two launches; a row's bits depend neither on its batch nor on its place in it"""
    sos = C.cascade(2)
    lens = [300 + 7 * b for b in range(64)] + [O.TILE + 9]
    rows = [C.speech_like(n) for n in lens]
    X, ns = C.padded(rows)
    got = run(engine, X, sos, n_samples=ns)
    for b in (0, 1, 31, 63, 64):
        assert C.same(got[b, :lens[b]], want(rows[b], sos)), b
    alone = {b: run(engine, rows[b][None], sos)[0] for b in (0, 63, 64)}
    three, ns3 = C.padded([rows[64], rows[0], rows[63]])
    moved = run(engine, three, sos, n_samples=ns3, in_place=False)
    for place, b in enumerate((64, 0, 63)):
        assert np.array_equal(C.bits(got[b, :lens[b]]), C.bits(alone[b]))
        assert np.array_equal(C.bits(moved[place, :lens[b]]), C.bits(alone[b]))


@pytest.mark.parametrize('S', [1, 8])
def test_non_finite_negative_zero_and_denormal_samples(engine, S):
    sos = C.cascade(S)
    for n in (257, O.TILE + 70):
        x = C.specials(n)
        w = want(x, sos)
        assert np.isnan(w[2 * n // 3 + 1:]).all() and np.isfinite(w[:2 * n // 3]).all()
        assert C.same(run(engine, x[None], sos)[0], w), (n, S)
    x = C.denormal(700)
    for k in ([[1.0, 0.0, 0.0, 0.0, 0.0]], [[0.5, 0.0, 0.0, 0.0, 0.0]], [[-1.0, 0.5, 0.25, -0.5, 0.25]]):
        got = run(engine, x[None], k)[0]
        assert np.array_equal(C.bits(got), C.bits(want(x, k)))               # -0.0 and the denormals themselves, bit for bit
    assert np.array_equal(C.bits(run(engine, x[None], [[1.0, 0.0, 0.0, 0.0, 0.0]])[0]), C.bits(x))


@pytest.mark.parametrize('off_in,off_out', [(1, 1), (2, 3), (3, 0), (0, 2)])
def test_buffers_off_a_16_byte_boundary(engine, off_in, off_out):
    """the rows start 4, 8 or 12 bytes behind a 16-byte boundary, in place (equal offsets) and out of place; N is odd, so every
    row of the batch has another alignment"""
    sos = C.cascade(2)
    B, N = 3, O.TILE + 259
    rows = [C.speech_like(n) for n in (N, 258, O.TILE - 1)]
    X, lens = C.padded(rows, N)
    room = B * N + 8
    d_in = engine.to_device(np.full(room, C.FILL, np.float32))
    d_out = d_in if off_in == off_out else engine.to_device(np.full(room, C.FILL, np.float32))
    try:
        flat = np.full(room, C.FILL, np.float32)
        flat[off_in:off_in + B * N] = X.reshape(-1)
        d_in.copy_from(flat)
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        engine._check(raw(engine, d_in.data_ptr() + 4 * off_in, d_out.data_ptr() + 4 * off_out, B, N, sos, n_samples=lens))
        got = d_out.to_host()
        assert np.all(got[:off_out] == C.FILL) and np.all(got[off_out + B * N:] == C.FILL)
        got = got[off_out:off_out + B * N].reshape(B, N)
        for b, r in enumerate(rows):
            assert C.same(got[b, :len(r)], want(r, sos)), b
            assert np.all(got[b, len(r):] == C.FILL), b
    finally:
        d_in.free()
        if d_out is not d_in:
            d_out.free()


def test_the_profile_stage_and_its_launches(engine):
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        run(engine, C.speech_like(700)[None], C.cascade(2))
        ms, launches = engine.profile_get('equalize')
        assert launches == 4 and ms > 0                       # the transition, and the three passes
        engine.profile_reset()
        X, ns = C.padded([C.speech_like(10 + b) for b in range(65)])
        run(engine, X, C.cascade(1), n_samples=ns)
        assert engine.profile_get('equalize')[1] == 7
    finally:
        engine.set_option('profile', 0)


def test_every_refusal_returns_its_code_and_enqueues_nothing(engine):
    H = pkg('_hip')
    sos = C.cascade(3)
    B, N = 2, 600
    X = np.stack([C.speech_like(N), C.speech_like(N, seed=5)])
    d, o = engine.to_device(X), engine.to_device(np.full((B, N), C.FILL, np.float32))
    p, q = d.data_ptr(), o.data_ptr()
    nan_k, inf_k, unstable, edge = sos.copy(), sos.copy(), sos.copy(), sos.copy()
    nan_k[1, 2], inf_k[2, 4], unstable[0, 3:], edge[1, 3:] = np.nan, np.inf, (0.0, 1.0), (1.5, 0.5)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        cases = {
            'wav': raw(engine, None, q, B, N, sos), 'out': raw(engine, p, None, B, N, sos), 'sos': raw(engine, p, q, B, N, None, S=3),
            'B': raw(engine, p, q, 0, N, sos), 'N': raw(engine, p, q, B, 0, sos),
            'n0': raw(engine, p, q, B, N, sos, n_samples=[N, 0]), 'n+': raw(engine, p, q, B, N, sos, n_samples=[N + 1, 5]),
            'S0': raw(engine, p, q, B, N, sos, S=0), 'S9': raw(engine, p, q, B, N, np.concatenate([sos] * 3), S=9),
            'nan': raw(engine, p, q, B, N, nan_k), 'inf': raw(engine, p, q, B, N, inf_k),
            'unstable': raw(engine, p, q, B, N, unstable), 'edge': raw(engine, p, q, B, N, edge),
            'align': raw(engine, p + 2, q, 1, N, sos), 'align_out': raw(engine, p, q + 1, 1, N, sos),
            'overlap': raw(engine, p, p + 4, 1, N, sos), 'overlap_behind': raw(engine, p + 4 * N, p + 4, 1, N, sos),
        }
        assert cases == dict.fromkeys(cases, H.TTS_ERR_INVALID), cases
        assert b'overlaps' in engine.lib.tts_last_error(engine.handle)
        assert engine.profile_get('equalize')[1] == 0
        assert np.array_equal(C.bits(o.to_host()), C.bits(np.full((B, N), C.FILL, np.float32))) and np.array_equal(C.bits(d.to_host()), C.bits(X))
        with pytest.raises(ValueError):
            engine.equalize(d, 'bright', n_samples=[N, N + 1])
        with pytest.raises(ValueError, match='stable'):
            engine.equalize(d, unstable)
        # the host-only entry points: design and profile limits are TTS_ERR_UNSUPPORTED, the rest TTS_ERR_INVALID
        five, forty, n = (ctypes.c_double * 5)(), (ctypes.c_double * 40)(), ctypes.c_int(0)
        lib = engine.lib
        assert lib.tts_equalizer_design(2, 22050, 1000.0, 1.0, 3.0, five) == H.TTS_OK
        assert lib.tts_equalizer_design(2, 7999, 1000.0, 1.0, 3.0, five) == lib.tts_equalizer_design(0, 22050, 11000.0, 1.0, 0.0, five) == \
            lib.tts_equalizer_design(1, 22050, 100.0, 31.0, 0.0, five) == lib.tts_equalizer_design(4, 22050, 100.0, 1.0, 25.0, five) == H.TTS_ERR_UNSUPPORTED
        assert lib.tts_equalizer_design(5, 22050, 1000.0, 1.0, 3.0, five) == lib.tts_equalizer_design(2, 22050, 1000.0, 1.0, 3.0, None) == H.TTS_ERR_INVALID
        assert lib.tts_equalizer_profile(b'bright', 8000, forty, ctypes.byref(n)) == H.TTS_ERR_UNSUPPORTED and b"'bright'" in lib.tts_last_error(None)
        assert lib.tts_equalizer_profile(b'loud', 22050, forty, ctypes.byref(n)) == lib.tts_equalizer_profile(b'warm', 22050, None, ctypes.byref(n)) == H.TTS_ERR_INVALID
        assert lib.tts_equalizer_max_sections() == O.MAX_SECTIONS
        # the setting refuses likewise and stays as it was
        assert lib.tts_set_equalizer(engine.handle, 1, None, 3) == H.TTS_ERR_INVALID
        assert lib.tts_set_equalizer(engine.handle, 1, unstable.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3) == H.TTS_ERR_INVALID
        assert engine._equalizer is None
    finally:
        engine.set_option('profile', 0)
        d.free()
        o.free()
