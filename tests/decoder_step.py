"""One step of the launch-per-layer decoder (csrc/decoder.hip: decoder_enqueue), checked from the decoder's own state (a
plain helper module, imported like gru_step.py).

With persistent_decoder = 0 a teacher-forced call zeroes the workspace dec.state and updates it in place, step by step:
att [B][A] | h_att [B][A] | h_dec[l] [B][U] (csrc/api_stages.hip: decoder_impl; the second copies behind them belong to the
persistent kernels and stay zero here).  A run of S steps therefore leaves state_S, the state step S of a run of S + 1
steps starts from -- provided the common steps of the two runs agree bit for bit, which the test asserts first.  `step`
computes that one step,

    pre-net(concat(x, att)) -> attention GRU -> Luong dot scores, softmax, context -> attention layer -> residual GRUs,

in float64 (the reference) or in float32 with the kernels' formulas (the host chain: sigmoidf_ / tanhf_ of tts_common.h,
the attention in TTS_ATT_PARTS parts with their own max and the merge exp(m_part - m) / sum of dec_gemm_body), from the
float32 keys the GPU computed, the memory, the teacher frame and the weights.  `assert_step` holds every new quantity to
4 x what the host chain reaches against float64 on the same state, per utterance and per channel.

MUTANTS are the step with one of the mistakes the kernels invite; tests/test_gru_step_host.py shows each at least twice
above the tolerance of some quantity."""
import numpy as np

import gru_step as S
from oracle import tacotron_oracle as O
from parity import assert_parity, slice_errors

BOUND_FACTOR = 4
SEPARATION = 2
ATT_PARTS = 4                      # TTS_ATT_PARTS (csrc/decoder.h)
TOL_FLOOR = BOUND_FACTOR * 2.0 ** -24      # a quantity the host chain gets exactly (one position: the alignment is 1) may still
TOL_CAP = 1e-5                             # be one rounding off on the GPU; and no tolerance may quietly grow past the cap
AXES = {'utt': 0, 'chan': 1}

MUTANTS = {
    'merge_without_shift': 'the attention parts merged without exp(m_part - m)',
    'previous_context': "the attention layer reads the previous step's context",
    'residual_dropped': 'the first residual GRU writes h, not y + h',
    'teacher_off_by_one': 'the teacher frame t r instead of t r - 1',
}


def defined(mutant, Ts, step):
    if mutant == 'merge_without_shift':
        return Ts > -(-Ts // ATT_PARTS)        # more than one part holds positions
    if mutant == 'previous_context' and Ts == 1:
        return False                           # one position: every step's context is that memory row
    return step >= 1                           # step 0 reads the GO frame and has no context before it


def zero_state(B, hp, dtype=np.float32):
    d = hp.decoder
    return dict(att=np.zeros((B, d.n_attention_units), dtype), h_att=np.zeros((B, d.n_attention_units), dtype),
                h_dec=[np.zeros((B, d.n_decoder_gru_units), dtype) for _ in range(d.n_gru_layers)])


def split_state(flat, B, hp):
    """the live copies of dec.state"""
    A, U, NL = hp.decoder.n_attention_units, hp.decoder.n_decoder_gru_units, hp.decoder.n_gru_layers
    flat = np.asarray(flat).reshape(-1)
    att, h_att = flat[:B * A].reshape(B, A), flat[B * A:2 * B * A].reshape(B, A)
    h_dec = [flat[B * (2 * A + l * U):B * (2 * A + (l + 1) * U)].reshape(B, U) for l in range(NL)]
    return dict(att=att, h_att=h_att, h_dec=h_dec)


def state_floats(B, hp):
    A, U, NL = hp.decoder.n_attention_units, hp.decoder.n_decoder_gru_units, hp.decoder.n_gru_layers
    return B * (A + 2 * (A + NL * U))


def teacher_frame(target, hp, step):
    """x of step `step`: zeros (GO) at 0, else frame step * r - 1 of target (B, n, r * n_mels)"""
    B = target.shape[0]
    if step == 0:
        return np.zeros((B, hp.n_mels), target.dtype)
    return target.reshape(B, -1, hp.n_mels)[:, step * hp.reduction - 1]


def _gru(x, h, w, scope, cudnn, f32):
    dt = np.float32 if f32 else np.float64
    sig = S._sigmoid32 if f32 else S._sigmoid64
    tanh = S._tanh32 if f32 else np.tanh
    U = h.shape[-1]
    g = sig((np.concatenate([x, h], -1) @ w[scope + '/gates/kernel'] + w[scope + '/gates/bias']).astype(dt))
    r, u = g[:, :U], g[:, U:]
    if cudnn:
        ci = x @ w[scope + '/candidate/input_projection/kernel'] + w[scope + '/candidate/input_projection/bias']
        ch = h @ w[scope + '/candidate/hidden_projection/kernel'] + w[scope + '/candidate/hidden_projection/bias']
        c = tanh((ci + r * ch).astype(dt))
    else:
        c = tanh((np.concatenate([x, r * h], -1) @ w[scope + '/candidate/kernel'] + w[scope + '/candidate/bias']).astype(dt))
    return (u * h + (1 - u) * c).astype(dt)


def _attend32(q, keys, memory, mutant):
    """dec_attention_kernel + the merge of dec_gemm_body / dec_align_finalize_kernel in float32: (alignment, context)"""
    B, Ts, _ = keys.shape
    Tp = -(-Ts // ATT_PARTS)
    score = np.einsum('bd,btd->bt', q, keys).astype(np.float32)
    e = np.zeros((B, Ts), np.float32)
    m = np.full((B, ATT_PARTS), -np.inf, np.float32)
    s = np.zeros((B, ATT_PARTS), np.float32)
    ctx = np.zeros((ATT_PARTS, B, memory.shape[-1]), np.float32)
    for p in range(ATT_PARTS):
        lo, hi = p * Tp, min(Ts, (p + 1) * Tp)
        if hi <= lo:
            continue
        m[:, p] = score[:, lo:hi].max(-1)
        e[:, lo:hi] = S._exp32(score[:, lo:hi] - m[:, p:p + 1])
        s[:, p] = e[:, lo:hi].sum(-1, dtype=np.float32)
        ctx[p] = np.einsum('bt,btd->bd', e[:, lo:hi], memory[:, lo:hi]).astype(np.float32)
    live = np.isfinite(m)
    shift = np.where(live, m - m.max(-1, keepdims=True), np.float32(0))
    coef = np.where(live, np.float32(1) if mutant == 'merge_without_shift' else S._exp32(shift), np.float32(0)).astype(np.float32)
    inv = (np.float32(1) / (coef * s).sum(-1, dtype=np.float32)).astype(np.float32)
    coef = coef * inv[:, None]
    a = e * np.repeat(coef, Tp, axis=1)[:, :Ts]
    return a.astype(np.float32), np.einsum('bp,pbd->bd', coef, ctx).astype(np.float32)


def step(state, x, keys, memory, w, hp, f32, mutant=None, prev_ctx=None):
    """One decoder step from `state` (att, h_att, h_dec) on the input frame x [B][n_mels]: a dict of the new att, h_att,
    h_dec, the alignment row [B][Ts], the top y [B][U] and the context.  float64, or float32 as the kernels compute."""
    dt = np.float32 if f32 else np.float64
    dec, cudnn = hp.decoder, bool(hp.force_cudnn)
    w = {k: v.astype(dt) for k, v in w.items() if k.startswith('decoder2/')}
    keys, memory, x = keys.astype(dt), memory.astype(dt), x.astype(dt)
    att, h_att = state['att'].astype(dt), state['h_att'].astype(dt)
    p = O.pre_net(np.concatenate([x, att], -1), w, O._ATT + '/pre_net', dec.pre_net_layers).astype(dt)
    h_att = _gru(p, h_att, w, O._ATT + '/gru_cell', cudnn, f32)
    if f32:
        a, ctx = _attend32(h_att, keys, memory, mutant)
    else:
        a = O.softmax_lastaxis(np.einsum('bd,btd->bt', h_att, keys))
        ctx = np.einsum('bt,btd->bd', a, memory)
    used = prev_ctx.astype(dt) if mutant == 'previous_context' else ctx
    att = (np.concatenate([h_att, used], -1) @ w[O._ATT + '/attention_layer/kernel']).astype(dt)
    y, h_dec = att, []
    for i in range(dec.n_gru_layers):
        h = _gru(y, state['h_dec'][i].astype(dt), w, '{}/cell_{}/gru_cell'.format(O._MRC, i + 1), cudnn, f32)
        h_dec.append(h)
        y = h if (mutant == 'residual_dropped' and i == 0) else (y + h).astype(dt)
    return dict(att=att, h_att=h_att, h_dec=h_dec, align=a, y=y, ctx=ctx)


def fields(out):
    """name -> [B][n] array of everything a step leaves behind"""
    f = {'att': out['att'], 'h_att': out['h_att'], 'align': out['align'], 'y': out['y']}
    f.update({'h_dec[{}]'.format(l): h for l, h in enumerate(out['h_dec'])})
    return f


def tolerances(state, x, keys, memory, w, hp):
    """({name: tolerance}, {name: host-chain error}, float64 step): 4 x the worst slice error of the host chain per quantity"""
    ref = step(state, x, keys, memory, w, hp, f32=False)
    host = fields(step(state, x, keys, memory, w, hp, f32=True))
    errs = {n: max(v[0] for v in slice_errors(host[n], r, AXES).values()) for n, r in fields(ref).items()}
    return {n: max(BOUND_FACTOR * e, TOL_FLOOR) for n, e in errs.items()}, errs, ref


def excess(got, state, x, keys, memory, w, hp):
    """{name: worst slice error of got / tolerance}"""
    tol, _, ref = tolerances(state, x, keys, memory, w, hp)
    r = fields(ref)
    return {n: max(v[0] for v in slice_errors(g, r[n], AXES).values()) / tol[n] for n, g in fields(got).items()}


def assert_step(label, got, state, x, keys, memory, w, hp):
    tol, errs, ref = tolerances(state, x, keys, memory, w, hp)
    r = fields(ref)
    print('decoder step {}: '.format(label) + ', '.join('{} tol {:.2e} (host {:.2e})'.format(n, tol[n], errs[n]) for n in tol))
    for n, g in fields(got).items():
        assert np.isfinite(g).all(), (label, n)
        assert tol[n] < TOL_CAP, (label, n, tol[n])
        assert_parity(g, r[n], AXES, tol[n], '{} {}'.format(label, n))
    return tol, errs


# ------------------------------------------------------------------------------------------------ cases
FORMS = S.FORMS
BATCHES = (1, 17)                  # one utterance; a second row tile of the small-M GEMM, with one live row
MEMORY_LENGTHS = (1, 5, 130)       # fewer positions than attention parts (three empty parts), 2 + 2 + 1 + 0, a real split
STEPS = (0, 1, 4)                  # the GO frame from the zero state, the first teacher frame, a state that has moved


def inputs(B, Ts, n_steps, hp):
    """(memory [B][Ts][2H] like a bi-GRU output, teacher target [B][n_steps][r n_mels]), float32"""
    rng = np.random.default_rng(7000 + 100 * B + Ts)
    memory = np.tanh(rng.normal(0.0, 0.6, (B, Ts, 2 * hp.encoder.n_gru_units))).astype(np.float32)
    return memory, rng.random((B, n_steps, hp.reduction * hp.n_mels)).astype(np.float32)


def host_keys(memory, w):
    return (memory.astype(np.float64) @ w['decoder2/memory_layer/kernel'].astype(np.float64)).astype(np.float32)


def host_run(memory, keys, target, w, hp, n_steps):
    """the float32 host chain from the zero state: (state after n_steps steps, context of the last one or zeros)"""
    B = memory.shape[0]
    state, ctx = zero_state(B, hp), np.zeros((B, memory.shape[-1]), np.float32)
    for t in range(n_steps):
        state = step(state, teacher_frame(target, hp, t), keys, memory, w, hp, f32=True)
        ctx = state['ctx']
    return state, ctx
