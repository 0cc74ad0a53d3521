"""One step of the bi-GRU of csrc/gru.hip, checked from the kernel's own state (a plain helper module, imported like
gemm_model.py).

The GPU's output row of step s - 1 IS the state the kernel read at step s, so every step of a recurrence can be recomputed
alone in float64 from (that row, the float32 xproj row, the weights) and held to a few float32 roundings: no accumulated
drift, nothing upstream.  `step_reference64` does that for every (b, t, direction, unit) at once, `step_model32` evaluates
the same steps in float32 numpy with the kernel's formulas and summation order, and `check_steps` holds
phi(GPU) to BOUND_FACTOR x phi(model), phi = max |got - ref| / D in units of u = 2^-24 (gemm_model.phi).

The error figure D, from csrc/tts_common.h (sigmoidf_, tanhf_) and csrc/gru.hip (GRU_STEP).  Every D_* below is an
absolute error in units of u; constant factors (how many roundings a 128-term sum really has) are left to phi, which is
measured on the model.

  pre-activation of a gate   z = x + sum_k h_k W_kj        fmas and adds, each within u of its own magnitude:
                             D_z = |x| + sum_k |h_k| |W_kj|
  sigmoidf_(z) = rcp(1 + __expf(-z)),  s = sigmoid(z)
      __expf(-z) is v_exp_f32 of the FLOAT32 product -z log2(e): rounding that product moves the exponent by |z| u, i.e.
      e = exp(-z) by a relative |z| u, and v_exp_f32 adds 1 u of its own; 1 + e rounds (u (1 + e)); v_rcp_f32 adds 1 u.
      With ds/de = -s^2 and s^2 e = s (1 - s):
                             D_s = s (1 - s) (D_z + |z| + 1) + 2 s              (slope s (1 - s) <= 1/4)
  candidate, GRUCell form    z_c = x_c + sum_k (r_k h_k) W_kj: the products r_k h_k and the sum round, and the error of
      every r_k enters through |h_k| |W_kj|:
                             D_zc = |x_c| + sum_k |r_k h_k| |W_kj| + sum_k D_s(r_k) |h_k| |W_kj|
  candidate, cuDNN form      z_c = x_c + r_j (sum_k h_k W_kj + b_j) =: x_c + r_j g_j
                             D_zc = |x_c| + r_j (sum_k |h_k| |W_kj| + |b_j|) + D_s(r_j) |g_j|
  tanhf_(z) = fma(-2, rcp(__expf(2 z) + 1), 1),  c = tanh(z),  q = 1 / (e + 1) = (1 - c) / 2
      e = exp(2 z) is off by a relative (2 |z| + 1) u (2 z is exact, the log2(e) product rounds), e + 1 and the rcp add
      2 u of q, the fma rounds to u |c|.  With dq/de = -q^2, 4 q^2 e = 1 - c^2:
                             D_c = (1 - c^2) (D_zc + |z_c| + 1/2) + 2 (1 - c) + |c|        (slope 1 - c^2 <= 1)
      (the 2 (1 - c) term is real: near c = -1 the formula subtracts 2 q ~ 2 from 1)
  blend                      h' = u h + (1 - u) c
                             D = |h - c| D_s(u) + (1 - u) D_c + |u h| + |(1 - u) c|

A result below the smallest normal float32 may be flushed to zero (v_rcp_f32 of a huge argument): D_s and D_c carry one
such quantum, FLUSH, which no element of any case comes near.  The slopes are evaluated at the float64 step (errors of
1e-6 do not move them); at saturation they vanish with the error they scale, which is what keeps the figure honest there.
Past |z| ~ 88 (gates) and ~ 44 (candidate) the float32 exponential overflows to inf and the kernel's rcp(inf) = 0 gives
the limit exactly; the model does the same.

`run_model32` is the model as a whole recurrence -- the host side of the whole-sequence tolerance -- and, with `mutant=`,
the kernel with ONE of the mistakes its construction invites (MUTANTS).  tests/test_gru_step_host.py shows that each of them
lies at least twice above the bound, by the very code path (`check_steps`) the GPU test uses."""
import numpy as np

import gemm_model as G
from parity import BTC, assert_parity, slice_errors

H = 128
BOUND_FACTOR = 4        # as tests/test_gpu_gemm_stages.py: another summation order within a K-quarter, hardware exp / rcp
SEPARATION = 2          # a mutant lies at least this far above the bound (tests/test_gemm_model_host.py)
SEQ_TOL_CAP = 1e-5
FORMS = ('grucell', 'cudnn')
FLUSH = 2.0 ** -126 / G.U

_F32 = np.float32
_ONE = np.float32(1)
_LOG2E = np.float32(1.4426950408889634)


# ------------------------------------------------------------------------------------------------ weights as packed
def input_projection(w, scope, n_in, form):
    """Wt [6H][n_in] and bias [6H] of the x-halves, [r | u | c] of fw, then of bw (csrc/api_handle.hip: pack_cbhg)"""
    rows, bias = [], []
    for d in ('fw', 'bw'):
        gs = '{}/gru/{}/gru_cell_{}'.format(scope, d, d)
        cand = gs + ('/candidate/input_projection' if form == 'cudnn' else '/candidate')
        rows += [w[gs + '/gates/kernel'][:n_in].T, w[cand + '/kernel'][:n_in].T]
        bias += [w[gs + '/gates/bias'], w[cand + '/bias']]
    return np.ascontiguousarray(np.concatenate(rows, 0), dtype=_F32), np.concatenate(bias).astype(_F32)


def recurrent_weights(w, scope, n_in, form):
    """[(W_gh [H][2H] with columns [r | u], W_ch [H][H], b_ch [H] or None)] for fw, bw: the recurrent halves"""
    out = []
    for d in ('fw', 'bw'):
        gs = '{}/gru/{}/gru_cell_{}'.format(scope, d, d)
        wg = w[gs + '/gates/kernel'][n_in:]
        if form == 'cudnn':
            wc, b = w[gs + '/candidate/hidden_projection/kernel'], w[gs + '/candidate/hidden_projection/bias'].astype(_F32)
        else:
            wc, b = w[gs + '/candidate/kernel'][n_in:], None
        out.append((np.ascontiguousarray(wg, dtype=_F32), np.ascontiguousarray(wc, dtype=_F32), b))
    return out


def _x_of(xproj, d):
    return xproj[..., 3 * H * d:3 * H * (d + 1)]


def h_prev(out, d):
    """the state every step read: the output row of the previous step in direction d, zero at the direction's first"""
    h = np.asarray(out)[..., H * d:H * (d + 1)]
    p = np.zeros_like(h)
    if d == 0:
        p[:, 1:] = h[:, :-1]
    else:
        p[:, :-1] = h[:, 1:]
    return p


# ------------------------------------------------------------------------------------------------ float64
def _sigmoid64(z):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-z))


def cell64(x, h, wd, form):
    """One cell step in float64 on x [..., 3H] = [r | u | c], h [..., H]: (h', D, pre-activations (z_r, z_u, z_c),
    (|x| and sum |h||W| of the three pre-activations)).  D as derived in the module docstring."""
    f = np.float64
    wg, wc = wd[0].astype(f), wd[1].astype(f)
    x, h = np.asarray(x, f), np.asarray(h, f)
    xr, xu, xc = x[..., :H], x[..., H:2 * H], x[..., 2 * H:]
    ah = np.abs(h)
    zg, ag = h @ wg, ah @ np.abs(wg)
    zr, zu = xr + zg[..., :H], xu + zg[..., H:]
    r, u = _sigmoid64(zr), _sigmoid64(zu)
    D_r = r * (1 - r) * (np.abs(xr) + ag[..., :H] + np.abs(zr) + 1) + 2 * r + FLUSH
    D_u = u * (1 - u) * (np.abs(xu) + ag[..., H:] + np.abs(zu) + 1) + 2 * u + FLUSH
    if form == 'cudnn':
        bch = wd[2].astype(f)
        g = h @ wc + bch
        rec_c = ah @ np.abs(wc)
        zc = xc + r * g
        D_zc = np.abs(xc) + r * (rec_c + np.abs(bch)) + D_r * np.abs(g)
    else:
        rh = r * h
        rec_c = np.abs(rh) @ np.abs(wc)
        zc = xc + rh @ wc
        D_zc = np.abs(xc) + rec_c + (D_r * ah) @ np.abs(wc)
    c = np.tanh(zc)
    D_c = (1 - c * c) * (D_zc + np.abs(zc) + 0.5) + 2 * (1 - c) + np.abs(c) + FLUSH
    hn = u * h + (1 - u) * c
    D = np.abs(h - c) * D_u + (1 - u) * D_c + np.abs(u * h) + np.abs((1 - u) * c)
    return hn, D, (zr, zu, zc), (np.abs(x), np.concatenate([ag, rec_c], -1))


def step_reference64(xproj, out, wrec, form, detail=False):
    """(ref, D), [B][T][2H] float64: every step recomputed alone from the output row before it (`out` is the GPU's)."""
    parts = [cell64(_x_of(xproj, d), h_prev(out, d), wrec[d], form) for d in (0, 1)]
    ref, D = (np.concatenate([p[i] for p in parts], -1) for i in (0, 1))
    return (ref, D, parts) if detail else (ref, D)


def sequence_reference64(xproj, wrec, form):
    """The whole recurrence in float64 from the float32 xproj: [B][T][2H]"""
    B, T = xproj.shape[:2]
    out = np.zeros((B, T, 2 * H))
    for d in (0, 1):
        h = np.zeros((B, H))
        for s in range(T):
            t = T - 1 - s if d else s
            h = cell64(_x_of(xproj, d)[:, t], h, wrec[d], form)[0]
            out[:, t, H * d:H * (d + 1)] = h
    return out


# ------------------------------------------------------------------------------------------------ float32 model
def _exp32(x):
    """__expf: v_exp_f32 (taken as correctly rounded) of the float32 product x log2(e)"""
    t = np.asarray(x, _F32) * _LOG2E
    with np.errstate(over='ignore', under='ignore'):
        return np.exp2(t.astype(np.float64)).astype(_F32)


def _sigmoid32(z):
    return (_ONE / (_ONE + _exp32(-z))).astype(_F32)


def _tanh32(z):
    q = (_ONE / (_exp32(_F32(2) * z) + _ONE)).astype(_F32)           # rcp(inf) = 0
    return (1.0 - 2.0 * q.astype(np.float64)).astype(_F32)           # one fma


def _dot32(h, w):
    """gru_dot32 + gru_sum4: per K-quarter four fma chains (k = 32 kq + 4 i + lane, i ascending), (a.x + a.y) + (b.x + b.y),
    then the quad (q0 + q1) + (q2 + q3).  A float32 product is exact in float64, so rounding the float64 sum once is an fma."""
    lead, N = h.shape[:-1], w.shape[1]
    hq = np.asarray(h, _F32).reshape(lead + (4, 8, 4)).astype(np.float64)
    wq = np.asarray(w, _F32).reshape(4, 8, 4, N).astype(np.float64)
    acc = np.zeros(lead + (4, 4, N), _F32)
    for i in range(8):
        acc = (acc.astype(np.float64) + hq[..., :, i, :, None] * wq[:, i]).astype(_F32)
    p = (acc[..., 0, :] + acc[..., 1, :]) + (acc[..., 2, :] + acc[..., 3, :])
    return (p[..., 0, :] + p[..., 1, :]) + (p[..., 2, :] + p[..., 3, :])


def cell32(x, hs, hreg, wd, form, mutant=None):
    """GRU_STEP in float32: hs is the state in LDS (what the dot products read), hreg the register copy (r * h, blend)"""
    wg, wc, bch = wd
    xr, xu, xc = x[..., :H], x[..., H:2 * H], x[..., 2 * H:]
    zg = _dot32(hs, wg)
    r, u = _sigmoid32(xr + zg[..., :H]), _sigmoid32(xu + zg[..., H:])
    if form == 'cudnn':
        g = _dot32(hs, wc)
        if mutant == 'h_for_rh':
            c = _tanh32(xc + (g + bch))
        elif mutant == 'bch_outside_r':
            c = _tanh32((xc + r * g) + bch)
        else:
            c = _tanh32(xc + r * (g + bch))
    else:
        c = _tanh32(xc + _dot32(hreg if mutant == 'h_for_rh' else r * hreg, wc))
    return (u * hreg + (_ONE - u) * c).astype(_F32)


def step_model32(xproj, out, wrec, form):
    """Every step alone, as step_reference64, in float32 with the kernel's formulas: [B][T][2H] float32"""
    xproj, out = np.asarray(xproj, _F32), np.asarray(out, _F32)
    return np.concatenate([cell32(_x_of(xproj, d), h_prev(out, d), h_prev(out, d), wrec[d], form) for d in (0, 1)], -1)


# name -> (what the kernel would have done, forms it exists in)
MUTANTS = {
    'x_next_at_s1': ('step s reads the x row of step s + 1 where s % 3 == 1 (xb1 <-> xc2)', FORMS),
    'x_next_in_tail': ('the same at the remainder steps behind the unrolled loop', FORMS),
    'bw_forward_x': ('the backward direction reads the x rows in forward order', FORMS),
    'h_for_rh': ('the candidate uses h in place of r * h', FORMS),
    'bch_outside_r': ('b_ch added outside r', ('cudnn',)),
    'quarters_swapped': ('the weights of K-quarters 1 and 2 exchanged', FORMS),
    'r_u_swapped': ('the r and u columns of the recurrent gate weights exchanged', FORMS),
    'stale_state': ('the dot products read the state of two steps ago (a ping-pong copy not flipped)', FORMS),
    'bf16_state': ('the state in LDS kept as bfloat16', FORMS),
    'nonzero_start': ('the first step starts from h = 0.01', FORMS),
}


def _bf16(x):
    b = np.ascontiguousarray(x, _F32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(_F32)


def touched(mutant, form, T, d, s):
    """does the mutant change what step s of direction d computes (given correct earlier rows)?"""
    if mutant == 'x_next_at_s1':
        return s % 3 == 1 and s + 1 < T
    if mutant == 'x_next_in_tail':
        return s >= 3 * (T // 3) and s + 1 < T
    if mutant == 'bw_forward_x':
        return d == 1 and 2 * s != T - 1
    if mutant == 'nonzero_start':
        return s == 0
    if mutant == 'bch_outside_r' or (mutant == 'h_for_rh' and form == 'cudnn'):
        return True
    return s >= 1               # the state is zero at step 0: nothing to exchange, round or gate (a stale one: step 1
                                # reads the zero start where it should read row 0)


def defined(mutant, form, T):
    return form in MUTANTS[mutant][1] and any(touched(mutant, form, T, d, s) for d in (0, 1) for s in range(T))


def run_model32(xproj, wrec, form, mutant=None):
    """The model as a whole recurrence, [B][T][2H] float32 -- with `mutant`, the kernel with that one mistake."""
    xproj = np.asarray(xproj, _F32)
    B, T = xproj.shape[:2]
    out = np.zeros((B, T, 2 * H), _F32)
    for d in (0, 1):
        wg, wc, bch = wrec[d]
        if mutant == 'quarters_swapped':
            perm = np.r_[0:32, 64:96, 32:64, 96:128]
            wg, wc = wg[perm], wc[perm]
        if mutant == 'r_u_swapped':
            wg = np.concatenate([wg[:, H:], wg[:, :H]], 1)
        wd = (np.ascontiguousarray(wg), np.ascontiguousarray(wc), bch)
        x = _x_of(xproj, d)
        h = np.full((B, H), 0.01 if mutant == 'nonzero_start' else 0.0, _F32)
        older = h
        for s in range(T):
            sx = s
            if (mutant == 'x_next_at_s1' and s % 3 == 1) or (mutant == 'x_next_in_tail' and s >= 3 * (T // 3)):
                sx = min(s + 1, T - 1)
            t = T - 1 - s if d else s
            tx = sx if (d == 0 or mutant == 'bw_forward_x') else T - 1 - sx
            hs = older if mutant == 'stale_state' else _bf16(h) if mutant == 'bf16_state' else h
            older = h
            h = cell32(x[:, tx], hs, h, wd, form, mutant)
            out[:, t, H * d:H * (d + 1)] = h
    return out


# ------------------------------------------------------------------------------------------------ the checks
def check_steps(label, xproj, out, wrec, form):
    """phi of `out` and of the model against the one-step float64 reference taken from `out` itself.  Prints both and
    the worst element; returns (phi GPU, phi model, (b, t, direction, unit, step))."""
    ref, D = step_reference64(xproj, out, wrec, form)
    m = step_model32(xproj, out, wrec, form)
    p_gpu, p_model = G.phi(out, ref, D), G.phi(m, ref, D)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.abs(np.asarray(out, np.float64) - ref) / D
    b, t, col = (int(i) for i in np.unravel_index(int(np.argmax(np.nan_to_num(q, nan=np.inf))), q.shape))
    d, unit = divmod(col, H)
    s = ref.shape[1] - 1 - t if d else t
    print('stage phi {}: GPU {:.3f} u, model {:.3f} u; worst at (b {}, t {}, {}, unit {}), step {} (s % 3 = {})'.format(
        label, p_gpu, p_model, b, t, 'bw' if d else 'fw', unit, s, s % 3))
    return p_gpu, p_model, (b, t, d, unit, s)


def assert_steps(label, xproj, out, wrec, form):
    p_gpu, p_model, worst = check_steps(label, xproj, out, wrec, form)
    assert np.isfinite(p_model) and p_gpu <= BOUND_FACTOR * p_model, (label, p_gpu, p_model, worst)
    return p_gpu, p_model


def sequence_tolerance(xproj, wrec, form):
    """(tolerance, float64 recurrence): 4 x the largest slice error of the float32 model run as a whole recurrence"""
    ref = sequence_reference64(xproj, wrec, form)
    host = run_model32(xproj, wrec, form)
    return BOUND_FACTOR * max(v[0] for v in slice_errors(host, ref, BTC).values()), ref


def assert_sequence(label, xproj, out, wrec, form):
    tol, ref = sequence_tolerance(xproj, wrec, form)
    assert tol < SEQ_TOL_CAP, (label, tol)
    assert_parity(out, ref, BTC, tol, label)
    return tol
