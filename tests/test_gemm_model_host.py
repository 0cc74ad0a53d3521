"""Host tests of the GEMM model (tests/gemm_model.py) and of the inputs the GPU tests use (tests/gemm_cases.py): the
split is exact, the documented arithmetic reaches the accuracy the kernel's comment records, and on every input of the
GPU accuracy test a kernel that has lost ONE of its six products lies at least twice above that test's bound."""
import numpy as np
import pytest

import gemm_cases as C
import gemm_model as G
from conftest import rel_l2

BOUND_FACTOR = 4        # tests/test_gpu_gemm.py: phi(GPU) <= 4 phi(model)
SEPARATION = 8          # twice that: where a lost product must lie at least


def test_split3_is_exact():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    rnd = bits.view(np.float32)
    rnd = rnd[np.isfinite(rnd) & (np.abs(rnd) > 2.0 ** -100)]      # all three terms normal
    pow2 = (2.0 ** np.arange(-100, 101)).astype(np.float32)
    # next to a bf16 boundary: the top 16 bits about to carry, the low 16 all ones / all zeros / one set
    tops = rng.integers(0x0D80, 0x7F00, 4000, dtype=np.uint64).astype(np.uint32) << np.uint32(16)
    edge = np.concatenate([tops | np.uint32(lo) for lo in (0xFFFF, 0x0000, 0x0001, 0x8000, 0x7FFF, 0x00FF, 0x0100, 0xFF00)]).view(np.float32)
    x = np.concatenate([rnd, -rnd[:1000], pow2, -pow2, edge, -edge, np.zeros(1, np.float32)])
    hi, mid, lo = G.split3(x)
    for t in (hi, mid, lo):
        assert not np.any(t.view(np.uint32) & np.uint32(0xFFFF)), 'a split term is not a bf16'
    s = ((hi.astype(np.float64) + mid.astype(np.float64)) + lo.astype(np.float64)).astype(np.float32)
    assert np.array_equal(s.view(np.uint32), x.view(np.uint32))
    # the truncations are one-sided and 8 bits apart
    nz = x != 0
    assert np.all(np.abs(mid[nz]) < 2.0 ** -7 * np.abs(x[nz])) and np.all(np.abs(lo[nz]) < 2.0 ** -15 * np.abs(x[nz]))


def test_k_order_visits_every_k_once():
    for case in C.CASES:
        B, T, Cin, ktaps, N, pool = case
        order = G.k_order(Cin, ktaps, pool)
        assert len(order) % G.BK == 0
        assert np.array_equal(np.sort(order[order >= 0]), np.arange(Cin * ktaps)), case
        tiles = G.slice_tiles(Cin * ktaps)
        assert tiles[0][0] == 0 and tiles[-1][1] * G.BK == len(order)
        assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(tiles, tiles[1:]))
    # the split-K cases that start a slice inside a tap group do
    starts = [t0 % 3 for t0, _ in G.slice_tiles(1376 * 3)]
    assert starts[1] == 1 and starts[2] == 2


def test_loader_paths_of_the_case_table():
    paths = {(G.loader_path(c[2], c[3], c[5]), bool(c[5]), G.splitk_slices(c[2] * c[3]) > 1) for c in C.CASES}
    for want in [('uniform', False, False), ('uniform', True, False), ('per_thread', False, False), ('general', False, False),
                 ('general', True, False), ('uniform', False, True), ('uniform', True, True), ('per_thread', False, True),
                 ('general', False, True)]:
        assert want in paths, want


@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_a_lost_product_is_far_above_the_bound(case, family):
    B, T, Cin, ktaps, N, pool = case
    x, w = C.data(case, family)
    ref, D = G.reference(x, w, ktaps, T, pool)
    outs = G.model_conv_many(x, w, ktaps, T, pool, G.ALL_MODELS)
    p = [G.phi(o, ref, D) for o in outs]
    print('model {} {}: phi {:.3f} u; one product lost: {}'.format(
        C.case_id(case), family, p[0], ' '.join('{} {:.1f}x'.format(n, q / max(p[0], 1e-300)) for n, q in zip(G.PAIR_NAMES, p[1:]))))
    assert np.isfinite(p[0])
    for name, q in zip(G.PAIR_NAMES, p[1:]):
        assert q >= SEPARATION * p[0], (name, q, p[0])


@pytest.mark.parametrize('case', C.LEGACY, ids=C.case_id)
def test_model_rel_l2_is_the_recorded_one(case):
    """csrc/gemm_f32.hip records 2.5e-7 rel-L2 against float64 on these shapes: the documented arithmetic is in that range."""
    B, T, Cin, ktaps, N, pool = case
    x, w = C.data(case, 'gauss')
    ref, _ = G.reference(x, w, ktaps, T, pool)
    e = rel_l2(G.model_conv(x, w, ktaps, T, pool), ref)
    print('model {}: rel-L2 {:.2e}'.format(C.case_id(case), e))
    assert 2e-8 < e < 5e-7


def test_exact_inputs_are_exact_in_the_model():
    """The routing, mirror and counting inputs give the float64 reference bit for bit under the documented arithmetic --
    and not with a product missing (routing / mirror), so the GPU tests that use them have no tolerance to hide in."""
    for case in [(2, 33, 80, 4, 33, 0), (3, 3, 128, 3, 64, 1), (2, 20, 1376, 3, 64, 0), (1, 1, 4, 1, 1, 0)]:
        B, T, Cin, ktaps, N, pool = case
        makers = [C.routing_inputs, C.counting_inputs] + ([] if pool else [C.mirror_inputs])
        for make in makers:
            x, w = make(case)
            ref, _ = G.reference(x, w, ktaps, T, pool)
            outs = G.model_conv_many(x, w, ktaps, T, pool, [G.PAIRS, G.dropped(1), G.dropped(4), G.dropped(0), G.dropped(3)])
            assert np.array_equal(outs[0].astype(np.float64), ref), (case, make.__name__)
            if make is C.routing_inputs:        # the terms of A: lo*hi and mid*hi carry them
                assert not np.array_equal(outs[1].astype(np.float64), ref) and not np.array_equal(outs[2].astype(np.float64), ref)
            if make is C.mirror_inputs:         # the terms of W: hi*lo and hi*mid
                assert not np.array_equal(outs[3].astype(np.float64), ref) and not np.array_equal(outs[4].astype(np.float64), ref)


def test_routing_ks_cover_the_seams():
    case = (2, 20, 1028, 4, 64, 0)
    ks = C.routing_ks(case, np.random.default_rng(0))
    assert len(ks) == 512 and len(set(ks.tolist())) == 512
    for k in (0, 1027, 1028, 4111, 4096, 16 * 32, 16 * 32 - 1):      # taps, the partial last tile, the first slice seam
        assert k in ks
    assert len(C.routing_ks((2, 33, 80, 4, 33, 0), np.random.default_rng(0))) == 320


def _tail_case():
    """What the CBHG tail of the encoder reads at (B, Ts) = (3, 50): projection 2 plus the pre-net residual, from a float32
    run of the oracle with the suite's weights, and the lifter / highway weights as the kernels hold them."""
    from conftest import pkg
    from oracle import tacotron_oracle as O
    hp = pkg('tacotron.params').ModelParams()
    w = pkg('tacotron.weights').synthetic_weights(0, hp)
    rng = np.random.default_rng(41)
    ids = rng.integers(2, 39, (3, 50)).astype(np.int32)
    st = {}
    O.encoder(ids, w, hp, st)
    p2 = (st['proj2'] + st['prenet']).astype(np.float32).reshape(150, -1)
    lifter = (G.weight_rows(w['encoder/lifter/kernel']), w['encoder/lifter/bias'])
    layers = []
    for l in range(hp.encoder.n_highway_layers):
        hs = 'encoder/highway_network/highway_layer_{}'.format(l)
        layers.append((G.weight_rows(w[hs + '/H/kernel']), w[hs + '/H/bias'], G.weight_rows(w[hs + '/T/kernel']), w[hs + '/T/bias']))
    return p2, lifter, layers


def test_a_lost_product_in_the_fused_tail_is_far_above_its_tolerance():
    """tests/test_gpu_gemm_stages.py holds the fused highway stack (its middle layers never leave LDS) to 4 x the slice
    errors of the host chain: the chain with one product lost in any single stage misses that at least twofold."""
    from parity import BTC, slice_errors
    p2, lifter, layers = _tail_case()
    shape = (3, 50, 128)
    ref = G.tail_chain64(p2, lifter, layers).reshape(shape)
    worst = lambda y: max(v[0] for v in slice_errors(y.reshape(shape), ref, BTC).values())
    tol = BOUND_FACTOR * worst(G.tail_chain_model(p2, lifter, layers))
    print('fused tail: tolerance {:.2e}'.format(tol))
    assert tol < 2e-6
    for stage in range(len(layers) + 1):
        ratios = [worst(G.tail_chain_model(p2, lifter, layers, lost=(stage, i))) / tol for i in range(len(G.PAIRS))]
        print('fused tail, stage {} without {}'.format(stage, ' '.join('{} {:.1f}x'.format(n, r) for n, r in zip(G.PAIR_NAMES, ratios))))
        assert min(ratios) >= 2, (stage, ratios)
