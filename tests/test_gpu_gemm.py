"""GPU tests of the GEMM / conv1d kernel on its own (tts_debug_gemm), over the case table of tests/gemm_cases.py: the
implicit im2col of TF 'SAME' conv1d (reference tacotron/layers.py:361-367, 432-437), the fused
max-pool(2,1,SAME) loader (layers.py:518-521; S4), every form of the loader (uniform / per-thread / general taps, even and
more than 16 taps, K below and off the tile depth), the XCD-aware tile map and split-K with its seams.

Three kinds of test.  ROUTING and COUNTING have no tolerance: inputs on which every correct order of the six bf16
products gives the float64 result exactly, so a k mapped to the wrong (tap, channel), a tap mask off by one at a sequence
end, a split term that does not arrive, a k visited twice or never at a slice seam cannot hide.  ACCURACY holds every
element to 4 x the error of the documented arithmetic itself (tests/gemm_model.py) on the same input, in units of
u = 2^-24 of sum_k |a||w|; tests/test_gemm_model_host.py shows that a kernel which has lost one of its six products lies at
least twice above that bound on each of these inputs."""
import numpy as np
import pytest

import gemm_cases as C
import gemm_model as G
from conftest import pkg, rel_l2
from parity import assert_parity, slice_errors

pytestmark = pytest.mark.gpu

BOUND_FACTOR = 4        # float32 against a bound: the project's convention (tests/test_audio_bounds_host.py)


def _run(engine, x, w, case):
    B, T, Cin, ktaps, N, pool = case
    M, N = x.shape[0], w.shape[0]
    dx, dw = engine.to_device(x), engine.to_device(w)
    dc = engine.empty((M, N))
    try:
        engine._check(engine.lib.tts_debug_gemm(engine.handle, dx.data_ptr(), dw.data_ptr(), dc.data_ptr(), M, N, Cin, ktaps,
                                                T, pool))
        return dc.to_host()
    finally:
        dx.free(); dw.free(); dc.free()


def _assert_exact(got, ref, label):
    """values, not bits: np.array_equal takes a signed zero for a zero"""
    bad = np.argwhere(got.astype(np.float64) != ref)
    assert np.array_equal(got.astype(np.float64), ref), '{}: {} of {} outputs differ, first at {}: got {!r}, exact {!r}'.format(
        label, len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_gemm_routing_terms_of_a(engine, case):
    """Each output is hi + mid + lo of ONE activation times a power of two: every (tap, channel) -> k map, every tap mask at
    a sequence end, the zero fill past M, N and K, the pool selects, and that all three split terms of A arrive."""
    B, T, Cin, ktaps, N, pool = case
    x, w = C.routing_inputs(case)
    ref, _ = G.reference(x, w, ktaps, T, pool)
    _assert_exact(_run(engine, x, w, case), ref, 'routing ' + C.case_id(case))


@pytest.mark.parametrize('case', [c for c in C.CASES if not c[5]], ids=C.case_id)
def test_gemm_routing_terms_of_w(engine, case):
    """The mirror image: each output is at most one full-significand weight times a power of two."""
    B, T, Cin, ktaps, N, pool = case
    x, w = C.mirror_inputs(case)
    ref, _ = G.reference(x, w, ktaps, T, pool)
    _assert_exact(_run(engine, x, w, case), ref, 'mirror ' + C.case_id(case))


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_gemm_counting(engine, case):
    """Small integers, bf16-exact: the result is the int64 product, whatever the order -- every k exactly once."""
    B, T, Cin, ktaps, N, pool = case
    x, w = C.counting_inputs(case)
    ref = G.im2col(x, ktaps, T, pool).astype(np.int64) @ w.astype(np.int64).T
    assert np.abs(ref).max() < 2 ** 23
    _assert_exact(_run(engine, x, w, case), ref.astype(np.float64), 'counting ' + C.case_id(case))


@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_gemm_accuracy_against_the_model(engine, case, family):
    """phi(GPU) <= 4 phi(model), phi = max |got - ref| / sum_k |a'||w| in u = 2^-24, the model on the same input."""
    B, T, Cin, ktaps, N, pool = case
    x, w = C.data(case, family)
    ref, D = G.reference(x, w, ktaps, T, pool)
    p_model = G.phi(G.model_conv(x, w, ktaps, T, pool), ref, D)
    got = _run(engine, x, w, case)
    p_gpu = G.phi(got, ref, D)
    print('gemm phi {} {}: GPU {:.3f} u, model {:.3f} u, rel-L2 {:.2e}'.format(C.case_id(case), family, p_gpu, p_model, rel_l2(got, ref)))
    assert np.isfinite(got).all()
    assert p_gpu <= BOUND_FACTOR * p_model, (p_gpu, p_model)


@pytest.mark.parametrize('B,T,Cin,ktaps,N,pool', C.LEGACY)
def test_gemm_conv_matches_numpy(engine, B, T, Cin, ktaps, N, pool):
    """The six shapes the suite has always had, per row and column (tests/parity.py) beside the element bound above: the
    tolerance is 4 x the model's own figure in the same metric instead of a flat 1e-5."""
    case = (B, T, Cin, ktaps, N, pool)
    x, w = C.data(case, 'gauss')
    ref, _ = G.reference(x, w, ktaps, T, pool)
    model = G.model_conv(x, w, ktaps, T, pool)
    got = _run(engine, x, w, case)
    e, e_model = rel_l2(got, ref), rel_l2(model, ref)
    label = 'gemm B={} T={} Cin={} k={} N={} pool={}'.format(B, T, Cin, ktaps, N, pool)
    print('{}: rel-L2 {:.2e} (model {:.2e})'.format(label, e, e_model))
    assert e <= BOUND_FACTOR * e_model
    tol = BOUND_FACTOR * max(v[0] for v in slice_errors(model, ref, {'row': 0, 'col': 1}).values())
    assert tol < 5e-6
    assert_parity(got, ref, {'row': 0, 'col': 1}, tol, label)


@pytest.mark.parametrize('option', ['gemm_ps', 'gemm_presplit'])
def test_gemm_variant_options_are_refused(engine, option):
    """Round 5's two GEMM variants (measured, not faster: profiles/r05_experiment_gemm_presplit.txt) -- producer / consumer
    waves (`gemm_ps`) and pre-split weight images (`gemm_presplit`) -- are not in the library: their options are refused."""
    H = pkg('_hip')
    with pytest.raises(H.TtsError) as e:
        engine.set_option(option, 1)
    assert e.value.code == H.TTS_ERR_INVALID and 'unknown option' in str(e.value)
