"""One step of the launch-per-layer decoder (csrc/decoder.hip, persistent_decoder = 0) from the decoder's own state.

A teacher-forced run of S steps leaves state_S in the workspace dec.state (att | h_att | h_dec[l], updated in place:
decoder_enqueue uses the first copies only); a run of S + 1 steps on the same memory and the same first S teacher frames
goes through that very state -- the common steps of the two runs are asserted equal bit for bit -- and leaves state_{S+1},
alignments[S] and dec.yhist[:, S].  Step S is then recomputed alone in float64 from state_S, the float32 dec.keys, the
memory, the teacher frame and the weights (tests/decoder_step.py), and every new quantity -- att, h_att, h_dec[l], the
alignment row, y -- is held per utterance and per channel to 4 x what a float32 host chain of the same step reaches on the
same state, instead of the 1e-3 / 1e-4 the mel and the alignments have after S steps from the top.
tests/test_gru_step_host.py shows four plausible mistakes at least twice above these tolerances.

Global attention, both GRU forms; B = 1 and 17, Ts = 1 (three empty attention parts), 5 and 130, S = 0 (the GO frame from
the zero state), 1 and 4.  The weight-stationary and streamed persistent decoders keep their state in scratch of their
own and are out of scope: the oracle and bit-identity tests (test_gpu_persistent.py, test_gpu_teacher_forcing.py) tie them to this
form."""
import numpy as np
import pytest

import decoder_step as DS
import gru_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', params=DS.FORMS)
def form_engine(request):
    form = request.param
    eng = pkg().Engine(C.hparams_of(form))
    eng.load_weights(C.weights_of('plain', form))
    eng.set_option('persistent_decoder', 0)
    yield form, eng
    eng.close()


def run(eng, hp, memory, target):
    """(mel, alignments, dec.state, dec.yhist) of a teacher-forced run over target's steps"""
    B, n = target.shape[:2]
    assert eng.teacher_kernel_choice(B, memory.shape[1]) == 0
    mel, align = eng.decoder_forward_teacher(memory, np.ascontiguousarray(target))
    mel, align = mel.to_host(), align.to_host()
    state = eng.debug_workspace('dec.state', (DS.state_floats(B, hp),))
    yhist = eng.debug_workspace('dec.yhist', (B, n, hp.decoder.n_decoder_gru_units))
    return mel, align, state, yhist


@pytest.mark.parametrize('step', DS.STEPS)
@pytest.mark.parametrize('Ts', DS.MEMORY_LENGTHS)
@pytest.mark.parametrize('B', DS.BATCHES)
def test_decoder_step_from_its_own_state(form_engine, B, Ts, step):
    form, eng = form_engine
    hp, w = C.hparams_of(form), C.weights_of('plain', form)
    memory, target = DS.inputs(B, Ts, step + 1, hp)
    if step:
        mel0, align0, flat0, yhist0 = run(eng, hp, memory, target[:, :step])
        before = DS.split_state(flat0, B, hp)
    else:
        before = DS.zero_state(B, hp)
    mel1, align1, flat1, yhist1 = run(eng, hp, memory, target)
    keys = eng.debug_workspace('dec.keys', (B, Ts, hp.decoder.n_attention_units))
    if step:          # run S stands for the inside of run S + 1
        assert np.array_equal(mel1[:, :step], mel0) and np.array_equal(align1[:step], align0)
        assert np.array_equal(yhist1[:, :step], yhist0)
    half = B * (2 * hp.decoder.n_attention_units + hp.decoder.n_gru_layers * hp.decoder.n_decoder_gru_units)
    assert not flat1[half:].any()                 # the second copies are not this form's
    got = DS.split_state(flat1, B, hp)
    got.update(align=align1[step], y=yhist1[:, step])
    DS.assert_step('{} B{} Ts{} step {}'.format(form, B, Ts, step), got, before, DS.teacher_frame(target, hp, step), keys,
                   memory, w, hp)
