"""GPU: tts_join against tests/join_oracle.py, bit for bit, at the smallest shapes that can still go wrong (join_cases.py): B = 5 rows
of N = 2003 samples, `out` filled with a NaN pattern before every call, N_out no multiple of 4, fades of 0, 1, 7 and 64 samples,
pieces of 1, 2, 3, 2 fade - 1, 2 fade, 2 fade + 1 samples and one of three tiles and a sample (a tile is the 512 output samples
a workgroup writes), every kind of gap, one and three groups, NaN, Inf and -0.0 in the inside, the fades and the overlaps."""
import numpy as np
import pytest

import join_cases as C
import join_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def wavs(engine):
    """per (fade, G): the list, the host batch with its specials, the same on the device, N_out and the oracle's result"""
    out = {}
    base = C.batch()
    for fade in C.FADES:
        for G in (1, 3):
            pieces, groups = C.pieces_of(fade, G)
            x = C.with_specials(base, pieces)
            N_out = C.odd_n_out(pieces, groups, fade)
            want, n_out = O.join(x, pieces, groups, fade, N_out)
            out[fade, G] = dict(pieces=pieces, groups=groups, x=x, d=engine.to_device(x), N_out=N_out, want=want, n_out=n_out)
    yield out
    for c in out.values():
        c['d'].free()


def test_the_tile_and_the_limits(engine):
    assert engine.join_tile() == C.TILE and engine.join_max_pieces() == 4096 and engine.join_max_fade() == 1 << 20
    for fade in C.FADES:
        pieces, groups = C.pieces_of(fade, 3)
        counts = [q[2] for q in pieces]
        assert {1, 2, 3, 2 * fade + 1, 3 * C.TILE + 1} <= set(counts) and (fade == 0 or {2 * fade - 1, 2 * fade} <= set(counts))
        assert groups.count(1) == 1 and sorted(set(q[0] for q in pieces)) == [0, 1, 2, 4]
        gaps = [q[3] for q in pieces[:-1]]
        assert {0, 1, C.LARGE_GAP} <= set(gaps) and min(gaps) == -fade and (fade == 0 or -1 in gaps)   # -min(f_p, f_p+1) reaches the whole fade
        assert any(q[1] % 2 for q in pieces) and C.odd_n_out(pieces, groups, fade) % 4


@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('fade', C.FADES)
def test_join_is_the_oracle(engine, wavs, fade, G):
    c = wavs[fade, G]
    assert c['N_out'] % 4 and len(c['n_out']) == G
    if fade:
        assert np.isnan(c['want']).any() and (c['want'].view(np.uint32) == 0x80000000).any() and np.isinf(c['want']).any()
    for shift in (0, 1, 3):     # `out` on a 16-byte boundary, and 4 and 12 bytes behind one
        rc, got, around = C.raw_join(engine, c['d'], c['x'].shape, c['pieces'], c['groups'], fade, c['N_out'], shift)
        assert rc == 0, engine.lib.tts_last_error(engine.handle)
        assert (around == C.NAN_PATTERN).all()                                  # nothing outside out[G][N_out] is written
        assert not (got == C.NAN_PATTERN).any()                                 # ... and every element of it is
        C.assert_same(got, c['want'], (fade, G, shift))
    for g, n in enumerate(c['n_out']):
        assert not c['want'][g, n:].view(np.uint32).any()                      # +0.0 behind a group
    # the binding: a fresh (G, N_out) array with N_out rounded up to a multiple of 4, and the plan's lengths
    out, n_out = engine.join(c['d'], c['pieces'], c['groups'], fade)
    try:
        assert n_out.tolist() == c['n_out'] == engine.join_plan(c['x'].shape, c['pieces'], c['groups'], fade).tolist()
        assert out.shape == (G, -(-max(c['n_out']) // 4) * 4)
        host = out.to_host()
        C.assert_same(host[:, :max(c['n_out'])].copy().view(np.uint32), c['want'][:, :max(c['n_out'])], (fade, G, 'binding'))
        assert not host[:, max(c['n_out']):].view(np.uint32).any()
        rows = engine.download_rows(out, n_out)
        assert [len(r) for r in rows] == c['n_out']
        for g, r in enumerate(rows):
            C.assert_same(r.view(np.uint32), c['want'][g, :len(r)], (fade, G, 'rows'))
    finally:
        out.free()
    # a host batch is uploaded: the same
    out, _n = engine.join(c['x'], c['pieces'], c['groups'], fade, N_out=c['N_out'])
    C.assert_same(out.to_host().view(np.uint32), c['want'], (fade, G, 'host input'))
    out.free()


@pytest.mark.parametrize('fade', [7, 64])
def test_nan_and_inf_stay_where_they_contribute(engine, wavs, fade):
    """a NaN in an overlap is NaN in that one output sample; one call's NaN touches nothing else"""
    c = wavs[fade, 1]
    offsets, _n, f = O.plan(c['pieces'], c['groups'], fade)
    clean = C.batch()
    want_clean, _ = O.join(clean, c['pieces'], c['groups'], fade, c['N_out'])
    d = engine.to_device(clean)
    try:
        rc, got, _a = C.raw_join(engine, d, clean.shape, c['pieces'], c['groups'], fade, c['N_out'])
    finally:
        d.free()
    assert rc == 0 and not np.isnan(got.view(np.float32)).any()
    C.assert_same(got, want_clean, (fade, 'clean'))
    rc, got, _a = C.raw_join(engine, c['d'], c['x'].shape, c['pieces'], c['groups'], fade, c['N_out'])
    assert rc == 0
    got = got.view(np.float32)
    expected = np.zeros(got.shape, bool)                                        # the output samples a NaN source sample contributes to
    for p, (row, first, count, _gap) in enumerate(c['pieces']):
        expected[0, offsets[p]:offsets[p] + count] |= np.isnan(c['x'][row, first:first + count])
    assert expected.any() and np.isnan(got[expected]).all()
    # every other NaN is an overlap of +Inf and -Inf; there are overlaps that a NaN lies in
    two = np.zeros(got.shape[1], int)
    for p, (_row, _first, count, _gap) in enumerate(c['pieces']):
        two[offsets[p]:offsets[p] + count] += 1
    assert two.max() == 2 and (np.isnan(got[0]) & ~expected[0] <= (two == 2)).all()
    assert (expected[0] & (two == 2)).any() and (expected[0] & (two == 1)).any()
    # ... and they reach nothing else: every sample without a special contributor is the clean call's
    special = np.zeros(got.shape, bool)
    for p, (row, first, count, _gap) in enumerate(c['pieces']):
        src = c['x'][row, first:first + count]
        special[0, offsets[p]:offsets[p] + count] |= ~np.isfinite(src) | (src.view(np.uint32) == 0x80000000)
    assert np.array_equal(got.view(np.uint32)[~special], want_clean.view(np.uint32)[~special])


def test_the_list_reversed_into_two_calls_gives_the_same_bits_per_piece(engine, wavs):
    """the samples of a piece that no neighbour lies over do not depend on the piece's place in a list, nor on the call"""
    fade = 7
    c = wavs[fade, 3]
    pieces, groups = c['pieces'], c['groups']
    offsets, _n, _f = O.plan(pieces, groups, fade)
    _rc, whole, _a = C.raw_join(engine, c['d'], c['x'].shape, pieces, groups, fade, c['N_out'])
    P = len(pieces)
    back = [(q[0], q[1], q[2], 2) for q in reversed(pieces)]                     # (gaps of 2: no overlaps)
    seen = 0
    for part in (back[:P // 2], back[P // 2:]):
        n_out = sum(q[2] + 2 for q in part)
        rc, got, _a = C.raw_join(engine, c['d'], c['x'].shape, part, [0] * len(part), fade, n_out + 1)
        assert rc == 0
        o = 0
        for row, first, count, _gap in part:
            p = P - 1 - seen
            assert pieces[p][:3] == (row, first, count)
            under = -pieces[p - 1][3] if p > 0 and groups[p - 1] == groups[p] and pieces[p - 1][3] < 0 else 0
            over = -pieces[p][3] if p + 1 < P and groups[p + 1] == groups[p] and pieces[p][3] < 0 else 0
            a, b = under, count - over
            mine = got[0, o + a:o + b]
            theirs = whole[groups[p], offsets[p] + a:offsets[p] + b]
            nan = np.isnan(mine.view(np.float32))
            assert np.array_equal(nan, np.isnan(theirs.view(np.float32))) and np.array_equal(mine[~nan], theirs[~nan]), p
            o += count + 2
            seen += 1
    assert seen == P


def test_the_most_pieces_and_one_beyond(engine):
    H = pkg('_hip')
    P = engine.join_max_pieces()
    x = C.batch()
    rng = np.random.default_rng(8)
    counts = rng.integers(1, 4, P + 1)
    pieces = [(int(rng.integers(0, C.B)), int(rng.integers(0, C.N - 3)), int(c), int(rng.integers(0, 3))) for c in counts]
    groups = np.minimum(np.arange(P + 1) // 700, 5).tolist()
    d = engine.to_device(x)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        N_out = C.odd_n_out(pieces[:P], groups[:P], 1)
        want, _n = O.join(x, pieces[:P], groups[:P], 1, N_out)
        rc, got, around = C.raw_join(engine, d, x.shape, pieces[:P], groups[:P], 1, N_out)
        assert rc == 0 and (around == C.NAN_PATTERN).all()
        C.assert_same(got, want, 'max pieces')
        assert engine.profile_get('join')[1] == P // 128 == 32                   # 128 pieces travel in a launch
        # one beyond: refused, and nothing is launched -- `out` keeps its pattern
        engine.profile_reset()
        rc, got, around = C.raw_join(engine, d, x.shape, pieces, groups, 1, N_out + 8)
        assert rc == H.TTS_ERR_INVALID and (got == C.NAN_PATTERN).all() and (around == C.NAN_PATTERN).all()
        assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'join: 4097 pieces are more than tts_join_max_pieces() = 4096'
        assert engine.profile_get('join') == (0.0, 0)
        with pytest.raises(ValueError):
            engine.join(d, pieces, groups, 1)
        assert engine.profile_get('join') == (0.0, 0)
        # a short list is one launch
        engine.join(d, pieces[:128], None, 1)[0].free()
        assert engine.profile_get('join')[1] == 1
        engine.join(d, pieces[:129], None, 1)[0].free()
        assert engine.profile_get('join')[1] == 3
    finally:
        engine.set_option('profile', 0)
        d.free()
