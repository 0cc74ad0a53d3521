"""GPU: tts_f0_compare (csrc/f0.hip) against tests/f0_oracle.py along paths that tts_dtw wrote -- 1 x 1, 1 x n, n x 1, 40 x 55 and a
ragged batch -- on F0 tracks with zeros, NaNs, equal values, a pair exactly at the 20 % edge and values one float apart.  The
counts and the sum of squared Hz differences are exact; the sum of squared cents goes through the device's log2 and is held to
|S - S64| <= 2e-12 sum |z_k| + 1e-15 S64 (include/sstts_hip.h)."""
import numpy as np
import pytest

import f0_cases as K
import f0_oracle as Y

pytestmark = pytest.mark.gpu


def _paths(engine, lens, Ta, Tb, seed=0):
    """paths of tts_dtw for pairs of the given lengths, on features that follow the tracks' index: (B, Ta + Tb - 1, 2)"""
    rng = np.random.default_rng(seed)
    B = len(lens)
    a = rng.standard_normal((B, Ta, 3)).astype(np.float32)
    b = rng.standard_normal((B, Tb, 3)).astype(np.float32)
    for p, (na, nb) in enumerate(lens):     # b is a warped copy of a, so the path wanders round the diagonal
        at = np.minimum((np.arange(nb) * na) // max(nb, 1), na - 1)
        b[p, :nb] = a[p, at] + 0.05 * rng.standard_normal((nb, 3)).astype(np.float32)
    cost, plen, path = engine.dtw(a, b, n_a=np.array([l[0] for l in lens], np.int32), n_b=np.array([l[1] for l in lens], np.int32),
                                  want_path=True)
    out = path.to_host().copy(), plen.to_host().copy()
    for d in (cost, plen, path):
        d.free()
    return out


def _check(engine, f0_a, f0_b, path, what):
    counts_d, sums_d = engine.f0_compare(f0_a, f0_b, path)
    counts, sums = counts_d.to_host().copy(), sums_d.to_host().copy()
    counts_d.free()
    sums_d.free()
    for p in range(f0_a.shape[0]):
        want_counts, s_hz, s_cents, abs_z = Y.compare(f0_a[p], f0_b[p], path[p])
        assert np.array_equal(counts[p], want_counts), (what, p, counts[p], want_counts)
        assert Y.same_bits(sums[p, 0], s_hz), (what, p, sums[p, 0], s_hz)
        bound = Y.cents_bound(s_cents, abs_z)
        err = abs(sums[p, 1] - s_cents)
        print('{} pair {}: steps {}, cents^2 sum {:.6e}, error {:.2e}, bound {:.2e}'.format(what, p, want_counts[0], s_cents, err, bound))
        assert err <= bound, (what, p, sums[p, 1], s_cents, err, bound)
    return counts, sums


@pytest.mark.parametrize('na,nb', [(1, 1), (1, 30), (30, 1), (40, 55)])
def test_along_a_dtw_path(engine, na, nb):
    path, plen = _paths(engine, [(na, nb)], na, nb, seed=na * 100 + nb)
    assert path.shape == (1, na + nb - 1, 2) and (path[0, plen[0]:] == -1).all()
    a, b = K.tracks(na + nb, na, nb)
    counts, _ = _check(engine, a[None], b[None], path, (na, nb))
    assert counts[0, 0] == plen[0]
    if (na, nb) == (40, 55):
        assert counts[0, 4] >= 1 and counts[0, 2] >= 1 and counts[0, 1] >= 20


def test_a_ragged_batch_and_the_marked_values(engine):
    lens = [(40, 55), (1, 9), (60, 2), (45, 45), (24, 24), (60, 55)]
    Ta, Tb = 60, 55
    path, plen = _paths(engine, lens, Ta, Tb, seed=9)
    A = np.full((len(lens), Ta), np.nan, np.float32)        # tracks behind a pair's lengths are poison: no path row names them
    Bm = np.full((len(lens), Tb), np.nan, np.float32)
    for p, (na, nb) in enumerate(lens):
        A[p, :na], Bm[p, :nb] = K.tracks(20 + p, na, nb)
    A[3, :45] = Bm[3, :45] = K.tracks(23, 45, 45)[0]        # a pair of equal tracks ...
    A[3, 14] = Bm[3, 14] = 150.0
    counts, sums = _check(engine, A, Bm, path, 'ragged')
    assert np.array_equal(counts[:, 0], plen)
    # ... differs nowhere it is voiced
    assert sums[3, 0] == 0.0 and sums[3, 1] == 0.0 and counts[3, 3] == 0
    # each pair alone, in buffers of its own size, along the same steps
    for p, (na, nb) in enumerate(lens):
        alone = _check(engine, A[p:p + 1, :na].copy(), Bm[p:p + 1, :nb].copy(), path[p:p + 1, :na + nb - 1].copy(), ('alone', p))
        assert np.array_equal(alone[0][0], counts[p]) and Y.same_bits(alone[1][0], sums[p])


def test_the_edge_of_a_gross_pitch_error_and_a_full_chunk_of_rows(engine):
    """the diagonal path of 130 equal-length frames: more than two chunks of 64 rows; the pair at the edge is no gross error, one
    float beyond it is"""
    n = 130
    a, b = K.tracks(77, n, n)
    path = K.diagonal_path(n, n, 2 * n - 1)[None]
    counts, _ = _check(engine, a[None], b[None], path, 'diagonal')
    assert counts[0, 0] == n
    edge = _check(engine, a[None, 17:19].copy(), b[None, 17:19].copy(), np.array([[[0, 0], [-1, -1]]], np.int32), 'edge')
    beyond = _check(engine, a[None, 17:19].copy(), b[None, 17:19].copy(), np.array([[[-1, -1], [1, 1]]], np.int32), 'beyond')
    assert edge[0][0].tolist() == [1, 1, 0, 0, 0] and beyond[0][0].tolist() == [1, 1, 0, 1, 0]
