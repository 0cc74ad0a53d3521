"""GPU: tts_watermark_embed and tts_watermark_detect (csrc/watermark.hip) against the numpy oracle of tests/watermark_oracle.py, bit for
bit: the embedder is individually rounded double operations with one rounding to float32, the detector integer sums.

The shapes are the smallest that reach every seam: lengths either side of an envelope block (64 samples), a row of several
streaming tiles (4096 samples) and of several correlation tiles (2048 chips), ragged batches with rows of 0, 1 and N samples, in
place and apart, buffers 4, 8 and 12 bytes off a 16-byte boundary; chips of 2, 6, 8 and 16 samples, symbols of 1, 5, 16 and 64 chips,
payloads of 1, 6, 8, 16 and 32 bits on rows that wrap them at least twice; 1, L, L + 1 and 64 offsets with the carrier cut at 0, inside
a chip, on a chip border and on a symbol border; NaN, +-Inf, -0.0 and denormal samples and an all-zero row."""
import ctypes

import numpy as np
import pytest

import watermark_cases as C
import watermark_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

_embedded, _detected = {}, {}


def marked(x, p):
    """the oracle's marked row, computed once per input and parameter set"""
    key = (np.asarray(x, np.float32).tobytes(), tuple(p))
    if key not in _embedded:
        _embedded[key] = O.embed(x, p)[0]
    return _embedded[key]


def found(r, p, D):
    key = (np.asarray(r, np.float32).tobytes(), tuple(p), D)
    if key not in _detected:
        _detected[key] = O.detect(r, p, D)
    return _detected[key]


def embed(engine, X, p, n_samples=None, in_place=True, out_fill=C.FILL, stats=False):
    """-> the result (B, N) float32 of host rows[, the records]"""
    X = np.ascontiguousarray(X, np.float32)
    d = engine.to_device(X)
    o = d if in_place else engine.to_device(np.full(X.shape, out_fill, np.float32))
    try:
        got = engine.watermark_embed(d, C.as_engine(p), n_samples=n_samples, out=None if in_place else o, stats=stats)
        rec = got[1] if stats else None
        assert (got[0] if stats else got) is o
        if not in_place:
            assert np.array_equal(C.bits(d.to_host()), C.bits(X))          # the input is read only
        return (o.to_host(), rec) if stats else o.to_host()
    finally:
        d.free()
        if not in_place:
            o.free()


def check_detection(rec, T, S, r, p, D, what):
    w = found(r, p, D)
    assert (int(rec['offset']), int(rec['n']), int(rec['score']), int(rec['energy']), int(rec['payload'])) == \
        (w.offset, len(r), w.score, w.energy, w.payload), what
    assert np.array_equal(T, w.T), what
    assert np.array_equal(S, w.S), what
    return w


def detect(engine, R, p, D, n_samples=None):
    return engine.watermark_detect(np.ascontiguousarray(R, np.float32), C.as_engine(p), offsets=D, n_samples=n_samples, want_scores=True, want_sums=True)


@pytest.mark.parametrize('name', sorted(C.SETS))
def test_every_length_is_the_oracle(engine, name):
    p = C.params(name)
    for n in (1, 63, 64, 65, 129, 2 * O.TILE + 301):
        x = C.voiced(n)
        got = embed(engine, x[None], p, in_place=n % 2 == 0)
        assert np.array_equal(C.bits(got[0]), C.bits(marked(x, p))), (name, n)
        if n > 192:
            assert np.sum(got[0] != x) > n // 3                              # ... and the row is marked
        else:
            assert np.array_equal(C.bits(got[0]), C.bits(x))                  # no block with a neighbour on either side
        for D in (1, p.chip + 1):
            rec, T, S = detect(engine, got, p, D)
            check_detection(rec[0], T[0], S[0], got[0], p, D, (name, n, D))


@pytest.mark.parametrize('name,cuts', [('default', (0, 3, 8, 40)), ('short', (0, 1, 2, 32)), ('wide', (0, 9, 16, 48)), ('byte', (5,)), ('narrow', (1, 2))])
def test_a_cut_row_is_found_at_its_offset_with_its_payload(engine, name, cuts):
    """the carrier cut at 0, inside a chip, on a chip border and on a symbol border, searched over 1, L, L + 1 and 64 offsets; a
    strong mark, so the oracle itself finds every cut that lies inside the offsets searched"""
    p = C.params(name, strength=0.25)
    n = 20000
    assert n >= 2 * p.payload_bits * p.chips_per_symbol * p.chip             # the payload wraps at least twice
    y = marked(C.voiced(n, seed=7), p)
    rows = [y[cut:] for cut in cuts]
    R, lens = C.padded(rows)
    for D in (1, p.chip, p.chip + 1, 64):
        rec, T, S = detect(engine, R, p, D, n_samples=lens)
        for b, cut in enumerate(cuts):
            w = check_detection(rec[b], T[b], S[b], rows[b], p, D, (name, cut, D))
            if cut < D:
                mask = (1 << p.payload_bits) - 1
                assert (w.offset, w.payload) == (cut, p.payload & mask), (name, cut, D)
                assert O.zeta(w.score, w.energy, p.payload_bits) > 2.0 * pkg('_hip').WM_THRESHOLD


@pytest.mark.parametrize('in_place', [True, False])
def test_a_ragged_batch_leaves_what_is_behind_its_rows(engine, in_place):
    p = C.params('byte')
    N = O.TILE + 300
    rows = [C.voiced(n) for n in (0, 1, N, 255, O.TILE)]
    X, lens = C.padded(rows, N)
    X[3, 255:] = np.float32(-0.0)                                            # (padding of another kind: -0.0 stays -0.0)
    got, stats = embed(engine, X, p, n_samples=lens, in_place=in_place, out_fill=np.float32(3.5), stats=True)
    for b, r in enumerate(rows):
        assert np.array_equal(C.bits(got[b, :len(r)]), C.bits(marked(r, p))), b
        assert np.array_equal(C.bits(got[b, len(r):]), C.bits(X[b, len(r):])), b       # apart: a copy; in place: untouched
        n, count, peak = O.embed_stats(r, p)
        assert (stats['n'][b], stats['marked'][b], stats['peak_out'][b]) == (n, count, peak), b
    rec, T, S = detect(engine, got, p, 9, n_samples=lens)
    for b, r in enumerate(rows):
        check_detection(rec[b], T[b], S[b], got[b, :len(r)], p, 9, b)
    assert rec['offset'][0] == 0 and rec['score'][0] == 0 and rec['energy'][0] == 0


def test_non_finite_negative_zero_and_denormal_samples(engine):
    for name in ('default', 'wide'):
        p = C.params(name)
        for n in (257, O.TILE + 70):
            x = C.specials(n)
            got = embed(engine, x[None], p)[0]
            want = marked(x, p)
            assert C.same(got, want) and np.array_equal(C.bits(got)[~np.isfinite(x)], C.bits(x)[~np.isfinite(x)])
            rec, T, S = detect(engine, got[None], p, 17)
            check_detection(rec[0], T[0], S[0], got, p, 17, (name, n))
        x = C.denormal(700)
        got = embed(engine, x[None], p)[0]
        assert np.array_equal(C.bits(got), C.bits(marked(x, p)))
        rec, T, S = detect(engine, x[None], p, 17)
        check_detection(rec[0], T[0], S[0], x, p, 17, name)


def test_no_strength_and_quiet_rows_come_back_as_their_own_bits(engine):
    x = C.specials(3000)
    p = C.params('default', strength=0.0)
    assert np.array_equal(C.bits(embed(engine, x[None], p)[0]), C.bits(x))
    assert np.array_equal(C.bits(embed(engine, x[None], p, in_place=False)[0]), C.bits(x))
    zeros = np.zeros(1000, np.float32)
    zeros[5::7] = -0.0
    got, stats = embed(engine, zeros[None], C.params('default'), stats=True)
    assert np.array_equal(C.bits(got[0]), C.bits(zeros)) and stats['marked'][0] == 0 and stats['peak_out'][0] == 0
    rec, T, S = detect(engine, zeros[None], C.params('default'), 64)
    assert rec['offset'][0] == 0 and rec['score'][0] == 0 and not T.any() and not S.any()


def test_a_tie_goes_to_the_lowest_offset(engine):
    """one sample under a non-zero envelope: v is 64 there and 0 elsewhere, so every offset scores 64"""
    x = np.zeros(192, np.float32)
    x[[10, 70, 130]] = 0.5
    p = C.params('narrow')
    assert O.v_of(x).tolist().count(64) == 1 and np.count_nonzero(O.v_of(x)) == 1
    rec, T, S = detect(engine, x[None], p, 64)
    assert np.all(T[0] == 64) and rec['offset'][0] == 0 and rec['score'][0] == 64 and rec['energy'][0] == 64 * 64
    check_detection(rec[0], T[0], S[0], x, p, 64, 'tie')


def test_a_rows_bits_depend_neither_on_its_batch_nor_on_what_ran_before(engine):
    """65 rows: two launches; a row alone, in another batch at another place, and behind a call with other parameters"""
    p = C.params('byte')
    lens = [300 + 7 * b for b in range(64)] + [O.TILE + 9]
    rows = [C.voiced(n) for n in lens]
    X, ns = C.padded(rows)
    got = embed(engine, X, p, n_samples=ns)
    rec, T, S = detect(engine, got, p, 20, n_samples=ns)
    for b in (0, 31, 63, 64):
        assert np.array_equal(C.bits(got[b, :lens[b]]), C.bits(marked(rows[b], p))), b
        check_detection(rec[b], T[b], S[b], got[b, :lens[b]], p, 20, b)
    detect(engine, got[:3], C.params('wide'), 64, n_samples=ns[:3])          # (leaves other sums in the workspace)
    three, ns3 = C.padded([got[64, :lens[64]], got[0, :lens[0]], got[63, :lens[63]]])
    rec3, T3, S3 = detect(engine, three, p, 20, n_samples=ns3)
    for place, b in enumerate((64, 0, 63)):
        alone = detect(engine, got[b:b + 1, :lens[b]], p, 20)
        for a, m, full in zip(alone, (rec3, T3, S3), (rec, T, S)):
            assert a[0].tobytes() == m[place].tobytes() == full[b].tobytes(), (place, b)


@pytest.mark.parametrize('off_in,off_out', [(1, 1), (2, 3), (3, 0), (0, 2)])
def test_buffers_off_a_16_byte_boundary(engine, off_in, off_out):
    """the rows start 4, 8 or 12 bytes behind a 16-byte boundary, in place (equal offsets) and apart; N is odd, so every row of
    the batch has another alignment"""
    H = pkg('_hip')
    p = C.params('default')
    B, N = 3, O.TILE + 259
    rows = [C.voiced(n) for n in (N, 258, O.TILE - 1)]
    X, lens = C.padded(rows, N)
    room = B * N + 8
    d_in = engine.to_device(np.full(room, C.FILL, np.float32))
    d_out = d_in if off_in == off_out else engine.to_device(np.full(room, C.FILL, np.float32))
    rec = engine.empty((B, 4), np.float64)
    try:
        flat = np.full(room, C.FILL, np.float32)
        flat[off_in:off_in + B * N] = X.reshape(-1)
        d_in.copy_from(flat)
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        w = H.TtsWatermark(*p)
        ns = lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        engine._check(engine.lib.tts_watermark_embed(engine.handle, d_in.data_ptr() + 4 * off_in, d_out.data_ptr() + 4 * off_out, B, N, ns,
                                                     ctypes.addressof(w), None))
        got = d_out.to_host()
        assert np.all(got[:off_out] == C.FILL) and np.all(got[off_out + B * N:] == C.FILL)
        engine._check(engine.lib.tts_watermark_detect(engine.handle, d_out.data_ptr() + 4 * off_out, B, N, ns, ctypes.addressof(w), 9, rec.data_ptr(),
                                                      None, None))
        records = rec.to_host().view(H.WATERMARK_DETECT_RECORD).reshape(B)
        got = got[off_out:off_out + B * N].reshape(B, N)
        for b, r in enumerate(rows):
            assert np.array_equal(C.bits(got[b, :len(r)]), C.bits(marked(r, p))), b
            assert np.all(got[b, len(r):] == C.FILL), b
            f = found(got[b, :len(r)], p, 9)
            assert (records['offset'][b], records['score'][b], records['energy'][b], records['payload'][b]) == (f.offset, f.score, f.energy, f.payload), b
    finally:
        d_in.free()
        rec.free()
        if d_out is not d_in:
            d_out.free()


def test_the_profile_stage_and_its_launches(engine):
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        embed(engine, C.voiced(700)[None], C.params('default'))
        ms, launches = engine.profile_get('watermark')
        assert launches == 2 and ms > 0                        # the blocks' maxima, the marked samples
        engine.profile_reset()
        X, ns = C.padded([C.voiced(200 + b) for b in range(65)])
        embed(engine, X, C.params('default'), n_samples=ns, stats=True)
        assert engine.profile_get('watermark')[1] == 6         # two launches of rows, with the records' third
        engine.profile_reset()
        detect(engine, X, C.params('default'), 9, n_samples=ns)
        assert engine.profile_get('watermark')[1] == 11        # the signs once, five per launch of rows
    finally:
        engine.set_option('profile', 0)


def test_every_refusal_returns_its_code_and_enqueues_nothing(engine):
    H = pkg('_hip')
    p = C.params('default')
    B, N = 2, 600
    X = np.stack([C.voiced(N), C.voiced(N, seed=5)])
    d, o = engine.to_device(X), engine.to_device(np.full((B, N), C.FILL, np.float32))
    rec = engine.empty((B, 4), np.float64)
    a, q, r = d.data_ptr(), o.data_ptr(), rec.data_ptr()

    def emb(p_wav, p_out, B_, N_, w, n_samples=None):
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, np.int32)
        s = None if w is None else H.TtsWatermark(*w)
        return engine.lib.tts_watermark_embed(engine.handle, p_wav, p_out, B_, N_, None if ns is None else ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              None if s is None else ctypes.addressof(s), None)

    def det(p_wav, B_, N_, w, D, p_rec, n_samples=None, scores=None, sums=None):
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, np.int32)
        s = None if w is None else H.TtsWatermark(*w)
        return engine.lib.tts_watermark_detect(engine.handle, p_wav, B_, N_, None if ns is None else ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               None if s is None else ctypes.addressof(s), D, p_rec, scores, sums)

    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        cases = {
            'wav': emb(None, q, B, N, p), 'out': emb(a, None, B, N, p), 'params': emb(a, q, B, N, None),
            'B': emb(a, q, 0, N, p), 'N': emb(a, q, B, 0, p),
            'n-': emb(a, q, B, N, p, n_samples=[N, -1]), 'n+': emb(a, q, B, N, p, n_samples=[N + 1, 5]),
            'P0': emb(a, q, B, N, p._replace(payload_bits=0)), 'P33': emb(a, q, B, N, p._replace(payload_bits=33)),
            'L0': emb(a, q, B, N, p._replace(chip=0)), 'L7': emb(a, q, B, N, p._replace(chip=7)), 'L18': emb(a, q, B, N, p._replace(chip=18)),
            'C0': emb(a, q, B, N, p._replace(chips_per_symbol=0)), 'C+': emb(a, q, B, N, p._replace(chips_per_symbol=65537)),
            'G-': emb(a, q, B, N, p._replace(strength=-0.01)), 'G+': emb(a, q, B, N, p._replace(strength=0.26)),
            'Gnan': emb(a, q, B, N, p._replace(strength=float('nan'))),
            'align': emb(a + 2, q, 1, N, p), 'align_out': emb(a, q + 1, 1, N, p),
            'overlap': emb(a, a + 4, 1, N, p), 'overlap_behind': emb(a + 4 * N, a + 4, 1, N, p),
            'd_wav': det(None, B, N, p, 9, r), 'd_rec': det(a, B, N, p, 9, None), 'd_params': det(a, B, N, None, 9, r),
            'd_B': det(a, 0, N, p, 9, r), 'd_N': det(a, B, 0, p, 9, r), 'd_n+': det(a, B, N, p, 9, r, n_samples=[N + 1, 5]),
            'd_L': det(a, B, N, p._replace(chip=3), 9, r), 'd_G': det(a, B, N, p._replace(strength=1.0), 9, r),
            'd_D0': det(a, B, N, p, 0, r), 'd_D+': det(a, B, N, p, 4097, r),
            'd_align': det(a + 2, 1, N, p, 9, r), 'd_align_rec': det(a, 1, N, p, 9, r + 4), 'd_align_scores': det(a, 1, N, p, 9, r, scores=q + 4),
            'd_align_sums': det(a, 1, N, p, 9, r, sums=q + 4),
        }
        assert cases == dict.fromkeys(cases, H.TTS_ERR_INVALID), cases
        assert b'8-byte aligned' in engine.lib.tts_last_error(engine.handle)
        assert engine.profile_get('watermark')[1] == 0
        assert np.array_equal(C.bits(o.to_host()), C.bits(np.full((B, N), C.FILL, np.float32))) and np.array_equal(C.bits(d.to_host()), C.bits(X))
        assert emb(a, q, B, N, p, n_samples=[0, N]) == H.TTS_OK             # (a row may hold nothing)
        assert engine.lib.tts_watermark_max_offsets() == H.WM_MAX_OFFSETS == O.MAX_OFFSETS
        with pytest.raises(ValueError):
            engine.watermark_embed(d, 5, n_samples=[N, N + 1])
        with pytest.raises(ValueError, match='chip'):
            engine.watermark_embed(d, (5, 0, 16, 7, 64, 0.02))
        # the setting refuses likewise and stays as it was
        bad = H.TtsWatermark(*p._replace(chip=5))
        assert engine.lib.tts_set_watermark(engine.handle, 1, None) == engine.lib.tts_set_watermark(engine.handle, 1, ctypes.addressof(bad)) == H.TTS_ERR_INVALID
        assert engine._watermark is None
    finally:
        engine.set_option('profile', 0)
        d.free()
        o.free()
        rec.free()
