"""GPU: tts_dtw (csrc/dtw.hip) against the numpy oracle of tests/dtw_oracle.py -- cost bit for bit, path_len and path integer for
integer (include/sstts_hip.h: every operation is an individually rounded double operation or an integer one) -- at shapes placed
round the kernel's cut of an anti-diagonal, with ties, in ragged batches whose padding is poison, with NaN frames, at the longest
sequences the call takes, and the refusal beyond them."""
import numpy as np
import pytest

import dtw_cases as K
import dtw_oracle as W
from conftest import pkg

pytestmark = pytest.mark.gpu


def _oracle(a, b, D=None):
    form = W.dtw_sequential if a.shape[0] * b.shape[0] <= 4000 else W.dtw_diagonals   # (tests/test_dtw_host.py holds them equal)
    return form(a, b, D)


def _run(engine, a, b, **kw):
    """one call on host arrays (B, T, K) -> host (cost, path_len, path)"""
    cost, plen, path = engine.dtw(a, b, want_path=True, **kw)
    out = cost.to_host(), plen.to_host(), path.to_host()
    for d in (cost, plen, path):
        d.free()
    return out


def _assert_pair(got, p, ref, rows, what):
    cost, plen, path = got
    assert W.same_bits(cost[p], ref[0]), (what, cost[p], ref[0])
    assert int(plen[p]) == ref[1], (what, plen[p], ref[1])
    assert np.array_equal(path[p], W.padded_path(ref[2], rows)), what


def test_shapes_round_the_cut(engine):
    t = engine.dtw_tile()
    assert 1 <= t <= engine.dtw_max_frames() and engine.dtw_max_frames() >= 2048
    for na, nb in K.shapes(t):
        a, b = K.random_pair(na * 7 + nb, na, nb, 13)
        got = _run(engine, a[None], b[None])
        _assert_pair(got, 0, _oracle(a, b), na + nb - 1, (na, nb))


@pytest.mark.parametrize('D', [1, 13, 16, 17, 128])
def test_frame_widths(engine, D):
    a, b = K.random_pair(D, 37, 53, D)
    _assert_pair(_run(engine, a[None], b[None]), 0, _oracle(a, b), 89, D)
    # the kernel's second slot of rows, in both of its forms (D <= 16 keeps a lane's rows of `a` in registers)
    if D in (13, 17):
        t = engine.dtw_tile()
        a, b = K.warped_pair(D, t + 1, t - 1, D)
        _assert_pair(_run(engine, a[None], b[None]), 0, _oracle(a, b), 2 * t - 1, ('two slots', D))


def test_leading_floats_of_wider_rows_and_the_offset_form(engine):
    """stride > D: only the first D floats of a row count; skip = 1 is the ptr + 1, D = K, stride = K + 1 form that leaves c0 out"""
    a, b = K.random_pair(11, 29, 41, 14)
    ref = _oracle(a[:, 1:], b[:, 1:], 13)
    _assert_pair(_run(engine, a[None], b[None], D=13, skip=1), 0, ref, 69, 'offset form')
    ref = _oracle(a, b, 5)
    poisoned_a, poisoned_b = a.copy(), b.copy()
    poisoned_a[:, 5:], poisoned_b[:, 5:] = np.nan, np.nan
    _assert_pair(_run(engine, poisoned_a[None], poisoned_b[None], D=5), 0, ref, 69, 'leading floats')


def test_the_tie_cases_hold_the_rule(engine):
    cases = K.tie_cases()
    names = sorted(cases)
    two = [n for n in names if cases[n][2] == 2]
    a = np.stack([cases[n][0] for n in two])
    b = np.stack([cases[n][1] for n in two])
    got = _run(engine, a, b)
    lens = []
    for p, n in enumerate(two):
        ref = W.dtw_sequential(*cases[n])
        _assert_pair(got, p, ref, 94, n)
        lens.append(ref[1])
    assert lens == [58, 63, 58, 59]   # (another order of the candidates gives 62 / 64 / 63 / 60: tests/test_dtw_host.py)
    one = [n for n in names if cases[n][2] == 1]
    got = _run(engine, np.stack([cases[n][0] for n in one]), np.stack([cases[n][1] for n in one]))
    for p, n in enumerate(one):
        _assert_pair(got, p, W.dtw_sequential(*cases[n]), 94, n)


def test_a_ragged_batch_equals_its_pairs_alone_and_elsewhere(engine):
    K_ = 13
    lens = [(37, 53), (1, 9), (60, 2), (45, 45), (9, 1)]
    Ta, Tb = 60, 53
    A = np.full((5, Ta, K_), np.nan, np.float32)     # padding frames are poison: never read
    Bm = np.full((5, Tb, K_), np.nan, np.float32)
    pairs = []
    for p, (na, nb) in enumerate(lens):
        a, b = K.warped_pair(40 + p, na, nb, K_) if min(na, nb) > 1 else K.random_pair(40 + p, na, nb, K_)
        A[p, :na], Bm[p, :nb] = a, b
        pairs.append((a, b))
    n_a = np.array([l[0] for l in lens], np.int32)
    n_b = np.array([l[1] for l in lens], np.int32)
    got = _run(engine, A, Bm, n_a=n_a, n_b=n_b)
    assert not np.isnan(got[0]).any()
    alone = []
    for p, (a, b) in enumerate(pairs):
        ref = _oracle(a, b)
        _assert_pair(got, p, ref, Ta + Tb - 1, ('batch', p))
        single = _run(engine, a[None], b[None])      # Ta, Tb = its own lengths
        _assert_pair(single, 0, ref, a.shape[0] + b.shape[0] - 1, ('alone', p))
        alone.append(ref)
    # the same pairs at other places of a batch that takes more than one launch, in longer buffers
    big, Ta2, Tb2 = 70, 64, 57
    places = [3, 63, 64, 17, 69]
    A2 = np.full((big, Ta2, K_), np.nan, np.float32)
    B2 = np.full((big, Tb2, K_), np.nan, np.float32)
    n_a2 = np.full(big, 5, np.int32)
    n_b2 = np.full(big, 6, np.int32)
    filler = K.random_pair(99, 5, 6, K_)
    A2[:, :5], B2[:, :6] = filler[0], filler[1]
    for p, at in enumerate(places):
        A2[at], B2[at] = np.nan, np.nan
        A2[at, :lens[p][0]], B2[at, :lens[p][1]] = pairs[p]
        n_a2[at], n_b2[at] = lens[p]
    got2 = _run(engine, A2, B2, n_a=n_a2, n_b=n_b2)
    for p, at in enumerate(places):
        _assert_pair(got2, at, alone[p], Ta2 + Tb2 - 1, ('elsewhere', p))
    fill_ref = _oracle(*filler)
    for at in (0, 62, 65):
        _assert_pair(got2, at, fill_ref, Ta2 + Tb2 - 1, ('filler', at))
    # without a path: the same cost and path_len
    cost, plen = engine.dtw(A2, B2, n_a=n_a2, n_b=n_b2)
    assert W.same_bits(cost.to_host(), got2[0]) and np.array_equal(plen.to_host(), got2[1])


def test_a_nan_frame_spoils_its_own_pair_only(engine):
    a = np.stack([K.random_pair(50 + p, 33, 47, 13)[0] for p in range(3)])
    b = np.stack([K.random_pair(50 + p, 33, 47, 13)[1] for p in range(3)])
    clean = _run(engine, a, b)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[1, 20, 12] = np.nan
    bad_b[2, 0, 0] = np.nan
    got = _run(engine, bad_a, bad_b)
    assert W.same_bits(got[0][0], clean[0][0]) and got[1][0] == clean[1][0] and np.array_equal(got[2][0], clean[2][0])
    for p in (1, 2):
        ref = W.dtw_sequential(bad_a[p], bad_b[p])
        assert np.isnan(got[0][p]) and np.isnan(ref[0])
        _assert_pair(got, p, ref, 79, ('nan', p))
    inf_a = a.copy()
    inf_a[0, 5, 3] = np.inf
    _assert_pair(_run(engine, inf_a, b), 0, W.dtw_sequential(inf_a[0], b[0]), 79, 'inf')


def test_the_longest_sequences(engine):
    n = engine.dtw_max_frames()
    a0, b0 = K.warped_pair(60, n, 2048, 13)
    a1, b1 = K.random_pair(61, n, 1999, 13)
    A = np.stack([a0, a1])
    Bm = np.full((2, 2048, 13), np.nan, np.float32)
    Bm[0], Bm[1, :1999] = b0, b1
    got = _run(engine, A, Bm, n_b=np.array([2048, 1999], np.int32))
    _assert_pair(got, 0, W.dtw_diagonals(a0, b0), n + 2047, 'longest, warped')
    _assert_pair(got, 1, W.dtw_diagonals(a1, b1), n + 2047, 'longest, random')


def test_refusal_above_the_limit_and_the_profile_stage(engine):
    H = pkg('_hip')
    n = engine.dtw_max_frames()
    a = np.zeros((1, n + 1, 2), np.float32)
    b = np.zeros((1, 3, 2), np.float32)
    for x, y in ((a, b), (b, a)):
        with pytest.raises(H.TtsError) as e:
            engine.dtw(x, y)
        assert e.value.code == H.TTS_ERR_UNSUPPORTED and str(n) in str(e.value)
    with pytest.raises(H.TtsError) as e:
        engine.dtw(np.zeros((1, 4, 129), np.float32), np.zeros((1, 4, 129), np.float32))
    assert e.value.code == H.TTS_ERR_UNSUPPORTED
    # a longer buffer is fine while the lengths are not
    a2, b2 = K.random_pair(70, 12, 9, 2)
    a[0, :12] = a2
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        got = _run(engine, a, b2[None], n_a=np.array([12], np.int32))
        ms, launches = engine.profile_get('dtw')
        assert launches == 1 and ms > 0
    finally:
        engine.set_option('profile', 0)
    _assert_pair(got, 0, _oracle(a2, b2), n + 1 + 9 - 1, 'after the refusals')
