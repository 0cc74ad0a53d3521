"""GPU: tts_encode (csrc/encode.hip) against the numpy oracle of tests/encode_oracle.py: every code and every record exactly equal.

The shapes are the smallest at which the kernel can go wrong: one sample, every length from 1 to 17 with the input and output
pointers at every residue of the packed stores (a row of N codes starts wherever the rows before it end, and both base pointers are
also offset by whole elements), lengths either side of a tile seam, rows that hold nothing, one sample or everything, more rows
than a launch takes, and seeds at both ends of 64 bits.  Every call writes into an output buffer with guard codes either side."""
import ctypes

import numpy as np
import pytest

import encode_cases as C
import encode_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 64                      # codes either side of the output
FORMS = [(f, d) for f in O.FORMATS for d in (O.NONE, O.TPDF)]
FORM_IDS = ['{}-{}'.format(O.NAMES[f], 'tpdf' if d else 'plain') for f, d in FORMS]


class Arena(object):
    """one input and one output buffer on the device, reused by every call of a test module"""

    def __init__(self, engine, floats, codes):
        self.engine = engine
        self.x = engine.empty((floats,), np.float32)
        self.y = engine.empty((2 * codes + 2 * GUARD,), np.uint8)
        self.st = engine.empty((256, 4), np.int32)

    def free(self):
        for a in (self.x, self.y, self.st):
            a.free()

    def encode(self, x, fmt, dither, seed=0, n_samples=None, in_off=0, out_off=0, keep_output=False):
        """-> (codes (B, N), records (B,)); the input starts ``in_off`` floats and the output ``out_off`` codes into their
        buffers; the guard codes either side of the output must come back as they were"""
        eng, lib = self.engine, self.engine.lib
        x = np.ascontiguousarray(x, np.float32)
        B, N = x.shape
        w, dt = O.WIDTH[fmt], O.DTYPE[fmt]
        assert (in_off + B * N) * 4 <= self.x.nbytes and (2 * GUARD + out_off + B * N) * w <= self.y.nbytes and B <= 256
        p_in = self.x.ptr + 4 * in_off
        p_guard = self.y.ptr + w * out_off
        p_out = p_guard + w * GUARD
        total = (B * N + 2 * GUARD) * w
        eng._check(lib.tts_memcpy_h2d(eng.handle, p_in, x.ctypes.data, x.nbytes))
        if not keep_output:
            fill = np.full(total, 0xA5, np.uint8)
            eng._check(lib.tts_memcpy_h2d(eng.handle, p_guard, fill.ctypes.data, total))
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, np.int32)
        ns_p = None if ns is None else ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        eng._check(lib.tts_encode(eng.handle, p_in, B, N, ns_p, fmt, dither, seed, p_out, self.st.ptr))
        raw = np.empty(total, np.uint8)
        eng._check(lib.tts_memcpy_d2h(eng.handle, raw.ctypes.data, p_guard, total))
        st = np.empty((B, 4), np.int32)
        eng._check(lib.tts_memcpy_d2h(eng.handle, st.ctypes.data, self.st.ptr, st.nbytes))
        assert np.all(raw[:GUARD * w] == 0xA5) and np.all(raw[-GUARD * w:] == 0xA5), 'a code was written outside the output'
        return raw[GUARD * w:-GUARD * w].view(dt).reshape(B, N).copy(), st.view(O.RECORD).reshape(B)


@pytest.fixture(scope='module')
def arena(engine):
    a = Arena(engine, 4 * O_TILE + 70000, 4 * O_TILE + 70000)
    yield a
    a.free()


O_TILE = 4096                   # tts_encode_tile(), asserted below


def _check(arena, x, fmt, dither, what, seed=0, n_samples=None, **where):
    got, st = arena.encode(x, fmt, dither, seed, n_samples, **where)
    want, wst = O.encode(x, fmt, dither, seed, n_samples)
    diff = np.argwhere(got != want)
    assert diff.size == 0, (what, diff[:6].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])
    assert C.same_records(st, wst), (what, st, wst)
    return got, st


def test_the_tile_is_what_the_tests_assume(engine):
    assert engine.lib.tts_encode_tile() == O_TILE == pkg('_hip').ENCODE_TILE


@pytest.mark.parametrize('fmt, dither', FORMS, ids=FORM_IDS)
def test_small_shapes_at_every_alignment(arena, fmt, dither):
    _check(arena, np.array([[0.37]], np.float32), fmt, dither, 'one sample')
    for N in range(1, 18):
        x = np.stack([C.speech_like(N, 1.1, seed=b) for b in range(3)])      # (rows N apart: three residues per call)
        for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 1), (2, 3), (3, 2)):
            _check(arena, x, fmt, dither, (N, in_off, out_off), seed=N, in_off=in_off, out_off=out_off)


@pytest.mark.parametrize('fmt, dither', FORMS, ids=FORM_IDS)
def test_across_the_tile_seams_ragged_rows_and_both_ends_of_the_seed(arena, fmt, dither):
    for N in (O_TILE + 1, 2 * O_TILE - 1):
        x = np.stack([C.speech_like(N, 1.05, seed=b) for b in range(2)])
        for in_off, out_off in ((0, 0), (1, 1), (3, 2)):
            _, st = _check(arena, x, fmt, dither, (N, in_off, out_off), seed=5, in_off=in_off, out_off=out_off)
        assert st['clipped'].min() > 0 and st['nans'].sum() == 0                # (the rows do go over full scale)
    # rows that hold nothing, one sample, everything: what lies behind a length is never read (NaN there counts nowhere)
    for N in (1, 5, O_TILE + 1):
        x = np.stack([C.speech_like(N, 0.9, seed=b) for b in range(3)])
        lens = np.array([0, 1, N], np.int32)
        for b in range(3):
            x[b, lens[b]:] = np.nan
        got, st = _check(arena, x, fmt, dither, ('ragged', N), seed=3, n_samples=lens)
        assert st['n'].tolist() == lens.tolist() and st['nans'].sum() == 0 and tuple(st[0]) == (0, 0, 0, 0)
        assert np.all(got[0] == O.SILENCE[fmt]) and np.all(got[1, 1:] == O.SILENCE[fmt])
    x = np.stack([C.speech_like(O_TILE + 9, 0.9, seed=b) for b in range(2)])
    a, _ = _check(arena, x, fmt, dither, 'seed 0', seed=0)
    b, _ = _check(arena, x, fmt, dither, 'seed 2^63 + 5', seed=2 ** 63 + 5)
    assert np.array_equal(a, b) == (dither == O.NONE)                            # the seed matters to the dither alone


@pytest.mark.parametrize('dither', [O.NONE, O.TPDF])
def test_more_rows_than_a_launch_takes(arena, dither):
    """130 rows: three launches; the dither is a function of the call's row, not the launch's"""
    x = np.stack([C.speech_like(257, 0.9, seed=b) for b in range(130)])
    lens = np.array([257 - b for b in range(130)], np.int32)
    for fmt in (O.S16, O.MULAW):
        _check(arena, x, fmt, dither, 'rows', seed=11, n_samples=lens)


def test_every_level_comes_back(arena):
    x = C.all_levels()[None]
    k = np.arange(-32768, 32768)
    got, st = _check(arena, x, O.S16, O.NONE, 'levels')
    assert np.array_equal(got[0], k) and tuple(st[0]) == (0, 0, 32768, 65536)
    assert np.array_equal(_check(arena, x, O.MULAW, O.NONE, 'levels')[0][0], O.lin2ulaw(k))
    assert np.array_equal(_check(arena, x, O.ALAW, O.NONE, 'levels')[0][0], O.lin2alaw(k))
    got8, _ = _check(arena, x, O.U8, O.NONE, 'levels')
    assert np.array_equal(got8[0, ::256], np.arange(256))
    # dithered, the levels move by at most one
    got, _ = _check(arena, x, O.S16, O.TPDF, 'levels', seed=1234)
    assert np.abs(got[0].astype(np.int64) - k).max() == 1


def test_the_special_values(arena):
    x, q, clipped, nans, peak = C.specials()
    got, st = _check(arena, x[None], O.S16, O.NONE, 'specials')
    assert np.array_equal(got[0], q) and tuple(st[0]) == (clipped, nans, peak, len(x))
    for fmt in (O.U8, O.MULAW, O.ALAW):
        _, st = _check(arena, x[None], fmt, O.NONE, 'specials')
        assert st['nans'][0] == nans and st['clipped'][0] >= clipped - 2 and st['n'][0] == len(x)
    # the non-finite samples count the same under dither (NaN + d is NaN, Inf + d is Inf)
    _, st = _check(arena, x[None], O.S16, O.TPDF, 'specials', seed=77)
    assert st['nans'][0] == nans and st['clipped'][0] >= 4


@pytest.mark.parametrize('fmt', O.FORMATS, ids=[O.NAMES[f] for f in O.FORMATS])
def test_padding_is_silence_and_a_second_call_overwrites_the_old_tail(arena, fmt):
    N = O_TILE + 37
    x = np.stack([C.speech_like(N, 0.9, seed=b) for b in range(2)])
    full, _ = _check(arena, x, fmt, O.TPDF, 'full', seed=2)
    assert np.any(full[:, N - 50:] != O.SILENCE[fmt])
    lens = np.array([N - 50, 3], np.int32)
    got, st = arena.encode(x, fmt, O.TPDF, 2, lens, keep_output=True)          # the same output buffer, untouched in between
    want, wst = O.encode(x, fmt, O.TPDF, 2, lens)
    assert np.array_equal(got, want) and C.same_records(st, wst)
    assert np.all(got[0, N - 50:] == O.SILENCE[fmt]) and np.all(got[1, 3:] == O.SILENCE[fmt])
    assert np.array_equal(got[0, :N - 50], full[0, :N - 50])                   # a sample's code does not depend on the length


def test_the_engines_forms_and_the_profile_stage(engine):
    x = np.stack([C.speech_like(999, 1.0, seed=b) for b in range(3)])
    lens = np.array([999, 0, 500], np.int32)
    want, wst = O.encode(x, O.ALAW, O.TPDF, 21, lens)
    codes, st = engine.encode(x, 'alaw', seed=21, n_samples=lens)               # host in, host out; TPDF by default
    assert isinstance(codes, np.ndarray) and codes.dtype == np.uint8 and np.array_equal(codes, want) and C.same_records(st, wst)
    d = engine.to_device(x)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        out, st = engine.encode(d, 'pcm16', dither=None)                        # device in, device out
        ms, launches = engine.profile_get('encode')
        assert launches == 2 and ms > 0                                         # the records and the pass
        assert out.dtype == np.int16 and out.shape == (3, 999) and np.array_equal(out.to_host(), O.encode(x, O.S16)[0])
        out.free()
    finally:
        engine.set_option('profile', 0)
        d.free()
    one, st = engine.encode(x[0], 'pcm8', dither=None)
    assert one.shape == (999,) and np.array_equal(one, O.encode(x[:1], O.U8)[0][0]) and st.shape == (1,)


def test_the_library_refuses_before_it_enqueues(engine):
    H = pkg('_hip')
    d = engine.empty((64,), np.float32)
    y = engine.empty((64,), np.int16)
    lib, h = engine.lib, engine.handle
    try:
        ok = lambda *a: lib.tts_encode(h, *a)
        assert ok(d.ptr, 2, 16, None, O.S16, 0, 0, y.ptr, None) == H.TTS_OK        # (no records: the stage's own)
        for args, text in (((d.ptr, 2, 16, None, O.F32, 0, 0, y.ptr, None), 'TTS_FMT_F32'),
                           ((d.ptr, 2, 16, None, 5, 0, 0, y.ptr, None), 'format'),
                           ((d.ptr, 2, 16, None, O.S16, 2, 0, y.ptr, None), 'dither'),
                           ((None, 2, 16, None, O.S16, 0, 0, y.ptr, None), 'NULL'),
                           ((d.ptr, 2, 16, None, O.S16, 0, 0, None, None), 'NULL'),
                           ((d.ptr, 0, 16, None, O.S16, 0, 0, y.ptr, None), 'B, N'),
                           ((d.ptr + 2, 2, 16, None, O.S16, 0, 0, y.ptr, None), 'aligned'),
                           ((d.ptr, 2, 16, None, O.S16, 0, 0, y.ptr + 1, None), 'aligned'),
                           ((d.ptr, 2, 16, None, O.S16, 0, 0, y.ptr, d.ptr + 2), 'aligned')):
            assert ok(*args) == H.TTS_ERR_INVALID, args
            assert text in lib.tts_last_error(h).decode(), (text, lib.tts_last_error(h))
        assert ok(d.ptr, 2, 16, None, O.MULAW, 0, 0, y.ptr + 1, None) == H.TTS_OK  # (a byte code is aligned anywhere)
        with pytest.raises(ValueError):
            engine.encode(d, 'pcm16', n_samples=[65])
        engine.synchronize()
    finally:
        d.free()
        y.free()
