"""The bi-GRU kernel (csrc/gru.hip) one step at a time, from its own state: the output row of step s - 1 is the state the
kernel read at step s, so every step is recomputed alone in float64 from (that row, the float32 xproj row the kernel read,
the weights) and held to 4 x the phi a float32 host model of the same step reaches on the same inputs (tests/gru_step.py,
where the error figure D is derived) -- the bound the GEMM stages have, with no drift and nothing upstream to dilute it.
Then the whole sequence against the float64 recurrence from the same xproj, to 4 x the drift of the host model.

Shapes and weight variants are tests/gru_cases.py's: every remainder of the three-way unroll, the clamped prefetch at T < 3,
several workgroups per direction, two long sequences; weights as the suite knows them, with the recurrent product
dominating, and with pre-activations past the overflow of the float32 exponentials.  tests/test_gru_step_host.py shows what
the bound is worth: each of ten plausible mistakes in the kernel lies at least twice above it.

Both CBHGs run with the fused_tail option at its default; the tail is not under test here (test_gpu_gemm_stages.py)."""
import numpy as np
import pytest

import gru_cases as C
import gru_step as S
from conftest import pkg

pytestmark = pytest.mark.gpu

H = S.H


@pytest.fixture(scope='module', params=[(v, f) for v in C.VARIANTS for f in S.FORMS], ids=lambda p: '{}-{}'.format(*p))
def variant_engine(request):
    variant, form = request.param
    eng = pkg().Engine(C.hparams_of(form))
    eng.load_weights(C.weights_of(variant, form))
    yield variant, form, eng
    eng.close()


def check_case(label, variant, form, net, xproj, out):
    wrec = C.wrec_of(net, variant, form)
    assert np.isfinite(xproj).all() and np.isfinite(out).all()
    S.assert_steps(label, xproj, out, wrec, form)
    S.assert_sequence(label, xproj, out, wrec, form)
    if variant == 'saturated':       # the GPU's xproj does reach past the overflow of both exponentials, in both signs
        _, _, parts = S.step_reference64(xproj, out, wrec, form, detail=True)
        gates = np.concatenate([np.concatenate(p[2][:2], -1) for p in parts], -1)
        cand = np.concatenate([p[2][2] for p in parts], -1)
        assert gates.max() > C.GATE_OVERFLOW and gates.min() < -C.GATE_OVERFLOW
        assert cand.max() > C.CAND_OVERFLOW and cand.min() < -C.CAND_OVERFLOW


@pytest.mark.parametrize('shape', C.SHAPES, ids=C.shape_id)
def test_postnet_gru_steps(variant_engine, shape):
    variant, form, eng = variant_engine
    B, T = shape
    lin = eng.postnet_forward(C.mel_input(shape)).to_host()
    xproj = eng.debug_workspace('post.xproj', (B, T, 6 * H))
    out = eng.debug_workspace('post.gru', (B, T, 2 * H))
    assert np.isfinite(lin).all()
    check_case('post.gru {} {} {}'.format(variant, form, C.shape_id(shape)), variant, form, 'post', xproj, out)


@pytest.mark.parametrize('shape', C.SHAPES, ids=C.shape_id)
def test_encoder_gru_steps(variant_engine, shape):
    variant, form, eng = variant_engine
    B, T = shape
    mem = eng.encoder_forward(C.ids_input(shape)).to_host()
    xproj = eng.debug_workspace('enc.xproj', (B, T, 6 * H))
    check_case('enc.gru {} {} {}'.format(variant, form, C.shape_id(shape)), variant, form, 'enc', xproj, mem)
