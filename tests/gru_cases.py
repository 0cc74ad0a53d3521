"""Shapes, weight variants and inputs of the one-step bi-GRU tests (a plain helper module, imported like arch_cases.py).
tests/test_gpu_gru_step.py runs csrc/gru.hip on them, tests/test_gru_step_host.py shows on the CPU that the variants are what
they claim to be and that the bound has teeth on these very inputs.

Every variant is a transform of synthetic_weights(SEED, hp) that touches only the GRU variables of the two CBHGs:

  plain      unchanged: gate bias 1, kernels of std 0.06 -- every gate near its centre
  recurrent  the recurrent rows of gates/kernel and candidate/kernel (hidden_projection/kernel) times RECURRENT_SCALE:
             sum |h||W| exceeds |x| in more than half of the pre-activations and |h| passes 0.9.  The scale is the
             largest of 1.5, 2, 2.5, 3, ... at which the recurrence is still stable: from 2.5 on the float32 model run as a
             whole sequence drifts from float64 by more than the 1e-5 the whole-sequence tolerance is capped at (T = 130),
             from 5 on it is chaotic (errors of order 1)
  saturated  the input rows and biases times SATURATED_SCALE: pre-activations of both signs beyond 45 in the candidate
             and 89 in the gates, where __expf(2 x) and __expf(-x) overflow in float32, in every case (T = 1 sets the
             scale: 256 gate pre-activations per utterance have to reach both thresholds).  The gate bias is scaled about
             its centre 1 (TF's initial value) -- scaled with it, every gate would saturate on the same side, u = 1, and
             the state would never leave zero

The scales were chosen on the CPU with the float64 recurrence on the oracle's highway outputs (host_xproj); the host test
asserts the conditions for every case."""
import copy
import functools

import numpy as np

from conftest import pkg
from oracle import tacotron_oracle as O

import gru_step as S

SEED = 7
# (B, T): every remainder of the three-way unroll, the clamped prefetch rows at T < 3, more than one workgroup per
# direction; two long enough for the state to leave its start-up regime
SHAPES = [(1, 1), (1, 2), (1, 3), (2, 4), (3, 5), (2, 6), (3, 7), (2, 64), (1, 130)]
VARIANTS = ('plain', 'recurrent', 'saturated')
NETS = ('post', 'enc')
SCOPE = {'post': 'post_process', 'enc': 'encoder'}
RECURRENT_SCALE = 2.0
SATURATED_SCALE = {'post': 320.0, 'enc': 520.0}
GATE_OVERFLOW, CAND_OVERFLOW = 89.0, 45.0


def shape_id(shape):
    return 'B{}-T{}'.format(*shape)


@functools.lru_cache(maxsize=None)
def hparams_of(form):
    hp = pkg('tacotron.params').ModelParams()
    hp.force_cudnn = form == 'cudnn'
    return hp


def n_in(net, form='grucell'):
    hp = hparams_of(form)
    return (hp.post if net == 'post' else hp.encoder).n_highway_units


@functools.lru_cache(maxsize=None)
def weights_of(variant, form):
    hp = hparams_of(form)
    w = copy.copy(pkg('tacotron.weights').synthetic_weights(SEED, hp))
    for net in NETS:
        U = n_in(net, form)
        for d in ('fw', 'bw'):
            gs = '{}/gru/{}/gru_cell_{}'.format(SCOPE[net], d, d)
            if form == 'cudnn':
                cand_in, cand_rec = gs + '/candidate/input_projection', gs + '/candidate/hidden_projection'
            else:
                cand_in = cand_rec = gs + '/candidate'
            names = {gs + '/gates/kernel', gs + '/gates/bias', cand_in + '/kernel', cand_in + '/bias', cand_rec + '/kernel'}
            for name in names:
                w[name] = w[name].copy()
            if variant == 'recurrent':
                w[gs + '/gates/kernel'][U:] *= np.float32(RECURRENT_SCALE)
                if form == 'cudnn':
                    w[cand_rec + '/kernel'] *= np.float32(RECURRENT_SCALE)
                else:
                    w[cand_rec + '/kernel'][U:] *= np.float32(RECURRENT_SCALE)
            elif variant == 'saturated':
                k = np.float32(SATURATED_SCALE[net])
                w[gs + '/gates/kernel'][:U] *= k
                w[gs + '/gates/bias'] = (np.float32(1) + k * (w[gs + '/gates/bias'] - np.float32(1))).astype(np.float32)
                w[cand_in + '/kernel'][:U] *= k
                w[cand_in + '/bias'] *= k
    return w


def mel_input(shape):
    B, T = shape
    return np.random.default_rng(500 + 10 * T + B).random((B, T, hparams_of('grucell').n_mels)).astype(np.float32)


def ids_input(shape):
    B, T = shape
    return np.random.default_rng(600 + 10 * T + B).integers(1, hparams_of('grucell').vocabulary_size, (B, T)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _highway(net, form, shape):
    """the input of the bi-GRU as the float64 oracle has it (the GRU variables do not enter: any variant)"""
    hp = hparams_of(form)
    w = {k: v.astype(np.float64) for k, v in weights_of('plain', form).items()}
    st = {}
    if net == 'post':
        O.post_process(mel_input(shape).astype(np.float64), w, hp, st)
    else:
        O.encoder(ids_input(shape), w, hp, st)
    return st['highway']


def host_xproj(net, variant, form, shape):
    """an xproj like the GPU's, [B][T][6H] float32: the oracle's highway output through the variant's input halves"""
    wt, b = S.input_projection(weights_of(variant, form), SCOPE[net], n_in(net, form), form)
    return (_highway(net, form, shape) @ wt.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)


def wrec_of(net, variant, form):
    return S.recurrent_weights(weights_of(variant, form), SCOPE[net], n_in(net, form), form)
