"""Host tests of the one-step bi-GRU checker (tests/gru_step.py) on the inputs of tests/test_gpu_gru_step.py
(tests/gru_cases.py): the checker and the oracle's bi_gru agree as independent implementations, the weight variants are what
they claim to be, and every mistake csrc/gru.hip invites by its construction (gru_step.MUTANTS), applied to the float32
model, lies at least twice above the bound the GPU test holds the kernel to -- by the same code path, check_steps -- with
the worst element reported at a step the mistake touched.  The same for one step of the launch-per-layer decoder
(tests/decoder_step.py, tests/test_gpu_decoder_step.py): its float64 step is the teacher-forced oracle's, and four mistakes in
the float32 host chain lie at least twice above the tolerance of some quantity of the step."""
import numpy as np
import pytest

import decoder_step as DS
import gru_cases as C
import gru_step as S
import teacher_oracle
from oracle import tacotron_oracle as O

H = S.H


@pytest.mark.parametrize('form', S.FORMS)
@pytest.mark.parametrize('T', [1, 2, 3, 7])
def test_checker_reproduces_the_oracle(form, T):
    """step_reference64 on O.bi_gru's own float64 output gives that output back, to 1e-12: both forms, both directions."""
    w32 = C.weights_of('plain', form)
    w = {k: v.astype(np.float64) for k, v in w32.items()}
    for net in C.NETS:
        U = C.n_in(net, form)
        x = np.random.default_rng(10 * T + U).normal(0.0, 1.0, (2, T, U))
        out = O.bi_gru(x, w, C.SCOPE[net] + '/gru', H, form == 'cudnn')
        wt, b = S.input_projection(w32, C.SCOPE[net], U, form)
        xproj = x @ wt.astype(np.float64).T + b.astype(np.float64)
        wrec = C.wrec_of(net, 'plain', form)
        ref, D = S.step_reference64(xproj, out, wrec, form)
        assert np.abs(ref - out).max() < 1e-12
        assert np.abs(S.sequence_reference64(xproj, wrec, form) - out).max() < 1e-12
        assert np.isfinite(D).all() and (D > 0).all()


def _pre_activations(x, wrec, form):
    """(float64 recurrence, gate pre-activations, candidate pre-activations, |x|, sum |h||W|) of one case, steps s >= 1 only
    in the last two (the state is zero at a direction's first step)"""
    seq = S.sequence_reference64(x, wrec, form)
    ref, _, parts = S.step_reference64(x, seq, wrec, form, detail=True)
    assert np.abs(ref - seq).max() < 1e-12
    gates = np.concatenate([np.concatenate(p[2][:2], -1) for p in parts], -1)
    cand = np.concatenate([p[2][2] for p in parts], -1)
    later = [np.s_[:, 1:], np.s_[:, :-1]]
    ax = np.concatenate([p[3][0][later[d]].ravel() for d, p in enumerate(parts)])
    ar = np.concatenate([p[3][1][later[d]].ravel() for d, p in enumerate(parts)])
    return seq, gates, cand, ax, ar


@pytest.mark.parametrize('net', C.NETS)
@pytest.mark.parametrize('form', S.FORMS)
@pytest.mark.parametrize('variant', C.VARIANTS)
def test_variants_are_what_they_claim(variant, form, net):
    wrec = C.wrec_of(net, variant, form)
    dominated, h_max = [], 0.0
    for shape in C.SHAPES:
        x = C.host_xproj(net, variant, form, shape)
        label = 'model {} {} {} {}'.format(net, variant, form, C.shape_id(shape))
        host = S.run_model32(x, wrec, form)
        assert np.isfinite(host).all()
        p_host, p_model, _ = S.check_steps(label, x, host, wrec, form)
        assert np.isfinite(p_model) and 0 < p_model < 4 and p_host <= S.BOUND_FACTOR * p_model
        tol, _ = S.sequence_tolerance(x, wrec, form)
        print('{}: whole-sequence tolerance {:.2e}'.format(label, tol))
        assert tol < S.SEQ_TOL_CAP
        seq, gates, cand, ax, ar = _pre_activations(x, wrec, form)
        h_max = max(h_max, float(np.abs(seq).max()))
        dominated.append(ar > ax)
        if variant == 'recurrent' and shape[1] >= 64:
            assert np.mean(ar > ax) > 0.5 and np.abs(seq).max() > 0.9, (shape, np.mean(ar > ax), np.abs(seq).max())
        if variant == 'saturated':
            assert gates.max() > C.GATE_OVERFLOW and gates.min() < -C.GATE_OVERFLOW, (shape, gates.min(), gates.max())
            assert cand.max() > C.CAND_OVERFLOW and cand.min() < -C.CAND_OVERFLOW, (shape, cand.min(), cand.max())
    frac = float(np.mean(np.concatenate(dominated)))
    print('{} {} {}: sum|h||W| > |x| in {:.0%} of the pre-activations behind a first step, max |h| {:.3f}'.format(
        net, variant, form, frac, h_max))
    if variant == 'recurrent':
        assert frac > 0.5 and h_max > 0.9


@pytest.mark.parametrize('variant,form,mutant', [(v, f, m) for v in C.VARIANTS for f in S.FORMS for m in S.MUTANTS
                                                 if f in S.MUTANTS[m][1]])       # b_ch exists in the cuDNN form only
def test_a_mutant_is_far_above_the_bound(variant, form, mutant):
    seen = 0
    for net in C.NETS:
        wrec = C.wrec_of(net, variant, form)
        for shape in C.SHAPES:
            T = shape[1]
            if not S.defined(mutant, form, T):
                continue
            x = C.host_xproj(net, variant, form, shape)
            out = S.run_model32(x, wrec, form, mutant)
            p_mut, p_model, (b, t, d, unit, s) = S.check_steps(
                '{} {} {} {} {}'.format(mutant, net, variant, form, C.shape_id(shape)), x, out, wrec, form)
            assert p_mut >= S.SEPARATION * S.BOUND_FACTOR * p_model, (net, shape, p_mut, p_model)
            assert S.touched(mutant, form, T, d, s), (net, shape, (b, t, d, unit, s))
            seen += 1
    assert seen >= 2 * 2          # both nets, and more than one shape each


def test_mutants_are_defined_where_expected():
    """the remainder-step mutant needs T % 3 == 2 (behind one remainder step the clamped prefetch row IS the right one),
    the s % 3 == 1 one T >= 3; one frame shows only the mistakes that do not need a state"""
    Ts = [T for _, T in C.SHAPES]
    assert [T for T in Ts if S.defined('x_next_in_tail', 'grucell', T)] == [2, 5]
    assert [T for T in Ts if S.defined('x_next_at_s1', 'grucell', T)] == [T for T in Ts if T >= 3]
    assert [m for m in S.MUTANTS if S.defined(m, 'cudnn', 1)] == ['h_for_rh', 'bch_outside_r', 'nonzero_start']
    assert [m for m in S.MUTANTS if S.defined(m, 'grucell', 1)] == ['nonzero_start']


# ---------------------------------------------------------------------------------------------------------- decoder step

@pytest.mark.parametrize('form', S.FORMS)
def test_decoder_step_reproduces_the_teacher_oracle(form):
    """tests/decoder_step.py's float64 step, iterated from the zero state, is teacher_oracle.decoder_teacher"""
    hp, w32 = C.hparams_of(form), C.weights_of('plain', form)
    w = {k: v.astype(np.float64) for k, v in w32.items()}
    B, Ts, n = 2, 5, 3
    memory, target = (a.astype(np.float64) for a in DS.inputs(B, Ts, n, hp))
    outs, aligns = teacher_oracle.decoder_teacher(memory, target, w, hp)
    keys = memory @ w['decoder2/memory_layer/kernel']
    state = DS.zero_state(B, hp, np.float64)
    for t in range(n):
        state = DS.step(state, DS.teacher_frame(target, hp, t), keys, memory, w, hp, f32=False)
        mel = state['y'] @ w['decoder2/decoder/output_projection_wrapper/kernel'] + w['decoder2/decoder/output_projection_wrapper/bias']
        assert np.abs(mel - outs[:, t]).max() < 1e-12 and np.abs(state['align'] - aligns[t]).max() < 1e-12


@pytest.mark.parametrize('mutant', list(DS.MUTANTS))
@pytest.mark.parametrize('form', S.FORMS)
def test_a_decoder_mutant_is_far_above_the_tolerance(form, mutant):
    """the float32 host chain with one mistake in step S, checked like the GPU's step (decoder_step.excess): some quantity
    of the step lies at least twice above its tolerance, on every case of tests/test_gpu_decoder_step.py that can show it"""
    hp, w = C.hparams_of(form), C.weights_of('plain', form)
    seen = 0
    for B in DS.BATCHES:
        for Ts in DS.MEMORY_LENGTHS:
            for step in DS.STEPS:
                if not DS.defined(mutant, Ts, step):
                    continue
                memory, target = DS.inputs(B, Ts, step + 1, hp)
                keys = DS.host_keys(memory, w)
                state, ctx = DS.host_run(memory, keys, target, w, hp, step)
                x = DS.teacher_frame(target, hp, step)
                xm = target.reshape(B, -1, hp.n_mels)[:, step * hp.reduction] if mutant == 'teacher_off_by_one' else x
                got = DS.step(state, xm, keys, memory, w, hp, f32=True, mutant=mutant, prev_ctx=ctx)
                ex = DS.excess(got, state, x, keys, memory, w, hp)
                clean = DS.excess(DS.step(state, x, keys, memory, w, hp, f32=True), state, x, keys, memory, w, hp)
                print('decoder {} {} B{} Ts{} step {}: worst {:.1f} x its tolerance ({}); the host chain {:.2f} x'.format(
                    mutant, form, B, Ts, step, max(ex.values()), max(ex, key=ex.get), max(clean.values())))
                assert max(clean.values()) <= 1.0 / DS.BOUND_FACTOR + 1e-12
                assert max(ex.values()) >= DS.SEPARATION, (B, Ts, step, ex)
                seen += 1
    assert seen >= 4
