"""GPU: tts_stoi (csrc/stoi.hip) against the numpy oracle of tests/stoi_oracle.py.  frames, kept, segments and kept_index equal
the oracle exactly; the envelopes lie within ``envelope_bound`` and the value within ``value_bound`` (DESIGN.md has the
derivation), in both modes; from the envelopes the device itself wrote, value and `degenerate` are the oracle's bits.  The rows
of tests/stoi_cases.py: lengths round a frame, kept frames round a segment, round the envelope workgroup's group and round the
segment workgroup's chunk, silence at the front, in the middle and at the end, NaN and Inf, pointers off a 16-byte boundary, a
ragged batch whose padding is poison, a batch beyond one launch, and the refusals."""
import numpy as np
import pytest

import stoi_cases as K
import stoi_oracle as S
from conftest import pkg

pytestmark = pytest.mark.gpu

MODES = (False, True)


def _bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _run(engine, ref, deg, extended, n_samples=None):
    """one call on host rows -> (records, kept_index, envelopes), host arrays"""
    return engine.stoi(np.atleast_2d(ref), np.atleast_2d(deg), n_samples=n_samples, extended=extended, want_index=True, want_envelopes=True)


def _check(got, b, o, extended, what, with_value):
    """row b of a call against the oracle dict ``o`` of that row"""
    rec, idx, env = got
    r = rec[b]
    kept = o['kept']
    assert (int(r['frames']), int(r['kept']), int(r['segments'])) == (o['frames'], kept, o['segments']), what
    assert np.array_equal(idx[b, :kept], o['index']), what
    X, Y = env[b, 0, :, :kept], env[b, 1, :, :kept]
    bx, by = S.envelope_bound(o)
    fine = np.isfinite(o['X']) & np.isfinite(o['Y'])
    assert np.array_equal(np.isfinite(X) & np.isfinite(Y), fine), what
    worst = max(float(np.max(np.abs(X - o['X'])[fine] / bx[fine], initial=0.0)), float(np.max(np.abs(Y - o['Y'])[fine] / by[fine], initial=0.0)))
    assert worst <= 1.0, (what, 'envelopes at %.3g of the bound' % worst)
    # steps 6 to 9 from the device's own envelopes: the oracle's bits
    value, degenerate, _ = S.from_envelopes(X, Y, extended)
    assert int(r['degenerate']) == degenerate, what
    assert _bits(r['value']) == _bits(value) or (np.isnan(r['value']) and np.isnan(value)), (what, r['value'], value)
    assert np.isnan(r['value']) == np.isnan(o['value']), what
    if with_value:
        assert S.centred_ratios(o, extended) >= 1e-3, what        # what the bound asks of its inputs
        bound = S.value_bound(o, extended)
        assert int(r['degenerate']) == o['degenerate'] == 0
        assert abs(float(r['value']) - o['value']) <= bound, (what, float(r['value']), o['value'], bound)
    return worst


@pytest.mark.parametrize('n', [255, 256, 383, 384])
def test_lengths_round_one_frame(engine, n):
    x = K.speech()[400:400 + n]            # inside the first burst
    y = K.degraded(x, 5)
    for extended in MODES:
        o = S.stoi(x, y, extended)
        assert o['frames'] == (0, 1, 1, 2)[(255, 256, 383, 384).index(n)] and o['kept'] == o['frames']
        got = _run(engine, x, y, extended)
        _check(got, 0, o, extended, n, False)
        assert np.isnan(got[0][0]['value'])


# kept frames round a segment (29 / 30 / 31), round the envelope workgroup's group and round the segment workgroup's chunk
KEPT = [K.GROUP - 1, K.GROUP, K.GROUP + 1, 29, 30, 31, K.SEG_CHUNK + 28, K.SEG_CHUNK + 29, K.SEG_CHUNK + 30]


@pytest.mark.parametrize('kept', KEPT)
def test_kept_frames_round_every_grouping(engine, kept):
    key = K.pattern_with_kept(kept, seed=3 if kept > 60 else 0)
    ref, deg = K.row(key)
    for extended in MODES:
        o = K.oracle(key, extended)
        assert o['kept'] == kept and o['frames'] == kept        # every frame of these rows is kept
        _check(_run(engine, ref, deg, extended), 0, o, extended, (kept, extended), kept >= 30)


@pytest.mark.parametrize('where', ['front', 'middle', 'end'])
def test_silence_at_the_front_in_the_middle_and_at_the_end(engine, where):
    key = K.pattern_with_kept(36, **{'front': dict(lead=5), 'middle': dict(gap_at=17, gap=6), 'end': dict(trail=5)}[where])
    ref, deg = K.row(key)
    for extended in MODES:
        o = K.oracle(key, extended)
        assert o['kept'] == 36 and o['frames'] > 36
        if where == 'middle':
            assert (np.diff(o['index']) > 1).sum() == 1      # the compaction joins two frames that were never neighbours
        _check(_run(engine, ref, deg, extended), 0, o, extended, (where, extended), True)


@pytest.mark.parametrize('snr', [10, 0])
def test_the_speech_like_row(engine, snr):
    key = ('speech', snr)
    ref, deg = K.row(key)
    for extended in MODES:
        _check(_run(engine, ref, deg, extended), 0, K.oracle(key, extended), extended, (snr, extended), True)


def test_nan_and_inf(engine):
    ref0, deg0 = K.row(('speech', 10))
    for extended in MODES:
        base = K.oracle(('speech', 10), extended)
        at = 128 * int(base['index'][40]) + 200
        # a NaN in ref: its frames drop out, the rest is measured
        ref = ref0.copy()
        ref[at] = np.nan
        o = S.stoi(ref, deg0, extended)
        assert o['kept'] == base['kept'] - 2 and np.isfinite(o['value'])
        got = _run(engine, ref, deg0, extended)
        _check(got, 0, o, extended, 'nan in ref', True)
        # a NaN, then an Inf, in deg: the counts stand, the value is NaN
        for bad in (np.nan, np.inf):
            deg = deg0.copy()
            deg[at] = bad
            o = S.stoi(ref0, deg, extended)
            assert o['kept'] == base['kept'] and np.isnan(o['value'])
            got = _run(engine, ref0, deg, extended)
            rec, idx, env = got
            assert (int(rec[0]['frames']), int(rec[0]['kept']), int(rec[0]['segments'])) == (o['frames'], o['kept'], o['segments'])
            assert np.array_equal(idx[0, :o['kept']], o['index']) and np.isnan(rec[0]['value'])
            # each signal has its own transform: the two frames that hold the sample have no finite Y, and X is untouched
            spoilt = ~np.isfinite(o['Y']).all(axis=0)
            assert spoilt.sum() == 2
            assert np.array_equal((~np.isfinite(env[0, 1, :, :o['kept']])).any(axis=0), spoilt)
            assert np.isfinite(env[0, 0, :, :o['kept']]).all()
        # an Inf in ref: its energy empties the row
        ref = ref0.copy()
        ref[at] = np.inf
        rec, _, _ = _run(engine, ref, deg0, extended)
        assert (int(rec[0]['frames']), int(rec[0]['kept']), int(rec[0]['segments'])) == (base['frames'], 0, 0) and np.isnan(rec[0]['value'])


def test_degenerate_terms_where_they_are_exact(engine):
    key = K.pattern_with_kept(33)
    ref, _ = K.row(key)
    silent = np.zeros_like(ref)
    # period 128: every frame away from the ends is the same bits, so every band of it is constant
    tile = (0.1 * np.random.default_rng(5).standard_normal(128)).astype(np.float32)
    periodic = np.tile(tile, 40)
    other = (0.1 * np.random.default_rng(6).standard_normal(len(periodic))).astype(np.float32)
    for extended in MODES:
        o = S.stoi(ref, silent, extended)
        rec, _, env = _run(engine, ref, silent, extended)
        assert int(rec[0]['degenerate']) == o['degenerate'] == 4 * (45 if extended else 15) and rec[0]['value'] == 0.0
        assert (env[0, 1] == 0.0).all()
        rec, _, env = _run(engine, periodic, other, extended)
        kept = int(rec[0]['kept'])
        assert kept == 39 and (env[0, 0, :, 1:kept - 1] == env[0, 0, :, 1:2]).all()
        # whether a centred norm of 30 equal numbers is 0.0 is a matter of their bits (the mean is a rounded sum over 30): the
        # count is the oracle's on the device's own envelopes
        value, degenerate, _ = S.from_envelopes(env[0, 0, :, :kept], env[0, 1, :, :kept], extended)
        assert int(rec[0]['degenerate']) == degenerate
        assert _bits(rec[0]['value']) == _bits(value) or (np.isnan(rec[0]['value']) and np.isnan(value))


class _View(object):
    """rows of a device buffer seen from a byte offset"""

    def __init__(self, base, offset, shape):
        self.base, self.offset, self.shape = base, offset, shape

    def data_ptr(self):
        return self.base.data_ptr() + self.offset


@pytest.mark.parametrize('off', [4, 8, 12])
def test_pointers_off_a_16_byte_boundary(engine, off):
    key = K.pattern_with_kept(36, gap_at=17, gap=6)
    ref, deg = K.row(key)
    n = len(ref)
    pad = np.full(off // 4, np.nan, np.float32)
    d_ref, d_deg = engine.to_device(np.concatenate([pad, ref])), engine.to_device(np.concatenate([pad, deg]))
    try:
        assert d_ref.data_ptr() % 16 == 0 and d_deg.data_ptr() % 16 == 0
        for extended in MODES:
            want = _run(engine, ref, deg, extended)
            got = engine.stoi(_View(d_ref, off, (1, n)), _View(d_deg, off, (1, n)), extended=extended, want_index=True, want_envelopes=True)
            assert K.same_results(got, want)
            _check(got, 0, K.oracle(key, extended), extended, (off, extended), True)
    finally:
        d_ref.free()
        d_deg.free()


def _ragged():
    keys = [K.pattern_with_kept(36, gap_at=17, gap=6), ('speech', 10), K.pattern_with_kept(29), K.pattern_with_kept(31), K.pattern_with_kept(5)]
    rows = [K.row(k) for k in keys]
    lens = np.array([len(r[0]) for r in rows], np.int32)
    N = int(lens.max()) + 77
    R, D = np.full((5, N), np.nan, np.float32), np.full((5, N), np.nan, np.float32)     # the padding is poison: never read
    for b, (r, d) in enumerate(rows):
        R[b, :len(r)], D[b, :len(d)] = r, d
    return keys, rows, lens, R, D


def test_a_ragged_batch_has_the_bits_of_its_rows_alone(engine):
    keys, rows, lens, R, D = _ragged()
    for extended in MODES:
        first = _run(engine, R, D, extended, n_samples=lens)
        engine.loudness(rows[1][0], 16000)                     # an unrelated call between the two
        second = _run(engine, R, D, extended, n_samples=lens)
        assert first[0].tobytes() == second[0].tobytes()
        for b, (key, (r, d)) in enumerate(zip(keys, rows)):
            alone = _run(engine, r, d, extended)
            kept = int(alone[0][0]['kept'])
            assert first[0][b].tobytes() == alone[0][0].tobytes(), (b, first[0][b], alone[0][0])
            assert np.array_equal(first[1][b, :kept], alone[1][0, :kept])
            assert _bits(first[2][b, :, :, :kept]).tolist() == _bits(alone[2][0, :, :, :kept]).tolist()
            _check(first, b, K.oracle(key, extended), extended, (b, extended), K.oracle(key, extended)['segments'] > 0)
        # without room for the indices and the envelopes: the same records
        plain = engine.stoi(R, D, n_samples=lens, extended=extended)
        assert plain.tobytes() == first[0].tobytes()


def test_a_batch_beyond_one_launch(engine):
    B = 66
    keys = [K.pattern_with_kept(30 + b % 2) for b in range(B)]
    rows = [K.row(k) for k in keys]
    lens = np.array([len(r[0]) for r in rows], np.int32)
    N = int(lens.max())
    R, D = np.full((B, N), np.nan, np.float32), np.full((B, N), np.nan, np.float32)
    for b, (r, d) in enumerate(rows):
        R[b, :len(r)], D[b, :len(d)] = r, d
    got = _run(engine, R, D, False, n_samples=lens)
    for b in (0, 1, 2, 63, 64, 65):
        alone = _run(engine, rows[b][0], rows[b][1], False)
        assert got[0][b].tobytes() == alone[0][0].tobytes(), b
        _check(got, b, K.oracle(keys[b], False), False, b, True)


def test_nothing_behind_the_kept_frames_is_touched(engine):
    H = pkg('_hip')
    key = K.pattern_with_kept(36, gap_at=17, gap=6)
    ref, deg = K.row(key)
    o = K.oracle(key, False)
    cap, kept = o['frames'], o['kept']
    assert kept < cap
    p, q = engine.to_device(ref[None]), engine.to_device(deg[None])
    rec = engine.empty((1, 3), np.float64)
    idx = engine.to_device(np.full((1, cap), -7, np.int32))
    env = engine.to_device(np.full((1, 2, 15, cap), -7.0, np.float64))
    try:
        engine._check(engine.lib.tts_stoi(engine.handle, p.data_ptr(), q.data_ptr(), 1, len(ref), None, 0, rec.data_ptr(), idx.data_ptr(),
                                          env.data_ptr()))
        got = (rec.to_host().view(H.STOI_RECORD).reshape(1), idx.to_host(), env.to_host())
        assert (got[1][0, kept:] == -7).all() and (got[2][0, :, :, kept:] == -7.0).all()
        _check(got, 0, o, False, 'prefilled buffers', True)
    finally:
        for a in (p, q, rec, idx, env):
            a.free()


def test_refusals_and_the_profile_stage(engine):
    H = pkg('_hip')
    ref, deg = K.row(K.pattern_with_kept(31))
    p, q = engine.to_device(ref[None]), engine.to_device(deg[None])
    rec = engine.empty((1, 3), np.float64)
    try:
        call = lambda *a: engine.lib.tts_stoi(engine.handle, *a)
        n = len(ref)
        most = 65535 * 128 + 256 + 127
        assert call(p.data_ptr(), q.data_ptr(), 1, most + 1, None, 0, rec.data_ptr(), None, None) == H.TTS_ERR_UNSUPPORTED
        assert 'tts_stoi_max_frames() = 65536' in engine.lib.tts_last_error(engine.handle).decode()
        for args in ((None, q.data_ptr(), 1, n, None, 0, rec.data_ptr(), None, None), (p.data_ptr(), None, 1, n, None, 0, rec.data_ptr(), None, None),
                     (p.data_ptr(), q.data_ptr(), 1, n, None, 0, None, None, None), (p.data_ptr(), q.data_ptr(), 0, n, None, 0, rec.data_ptr(), None, None),
                     (p.data_ptr(), q.data_ptr(), 1, 0, None, 0, rec.data_ptr(), None, None), (p.data_ptr(), q.data_ptr(), 1, n, None, 2, rec.data_ptr(), None, None),
                     (p.data_ptr() + 2, q.data_ptr(), 1, n - 1, None, 0, rec.data_ptr(), None, None),
                     (p.data_ptr(), q.data_ptr(), 1, n, None, 0, rec.data_ptr() + 4, None, None)):
            assert call(*args) == H.TTS_ERR_INVALID, args
            assert engine.lib.tts_last_error(engine.handle).decode().startswith('stoi: ')
    finally:
        for a in (p, q, rec):
            a.free()
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        got = _run(engine, ref, deg, False)
        ms, launches = engine.profile_get('stoi')
        assert launches == 5 and ms > 0
        _run(engine, np.stack([ref] * 65), np.stack([deg] * 65), True)
        assert engine.profile_get('stoi')[1] == 5 + 10                # five launches per 64 rows
    finally:
        engine.set_option('profile', 0)
    _check(got, 0, K.oracle(K.pattern_with_kept(31), False), False, 'after the refusals', True)
