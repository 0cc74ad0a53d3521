"""Every product GEMM of the two CBHG stacks, each from the float32 input the kernel itself read (the stage workspaces,
engine.debug_workspace): the epilogues (bias, relu, folded batch norm, residual, channel offset), the grouped conv-bank
launch, the embedding gather, split-K behind the max-pool loader, the final Dense, the attention keys and csrc/cbhg_tail.hip.
Nothing upstream dilutes or excuses a stage.

The figure is tests/gemm_model.py's phi with the epilogue folded into the scale:

    D = |scale| (sum_k |a||w| + |bias|) + |shift| + |residual|,      bound: 4 x phi(model GEMM + float32 numpy epilogue)

The batch norm is folded from the weights as tts_finalize_weights folds it -- in double, scale and shift each rounded to
float32 once -- so that the figure measures the kernel and not the fold.  tests/test_gemm_model_host.py shows what the bound
is worth: a GEMM that has lost one of its six products lies at least twice above it."""
import copy

import numpy as np
import pytest

import arch_cases
import gemm_model as G
from conftest import pkg
from parity import BTC, assert_parity, slice_errors

pytestmark = pytest.mark.gpu

BOUND_FACTOR = 4
BN_EPS = np.float64(np.float32(1e-3))
ENC_SHAPE = (3, 50)
POST_SHAPES = [(2, 77), (1, 1)]


def make_ids(rng, B, Ts):
    ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
    for b in range(B):
        L = int(rng.integers(max(2, Ts // 2), Ts))
        ids[b, L - 1] = 1
        ids[b, L:] = 0
    return ids


def _bn_name(i):
    return 'batch_normalization' if i == 0 else 'batch_normalization_{}'.format(i)


def fold_bn(w, scope, gamma):
    """(scale, shift) float32, folded in double and rounded once each (csrc/api_handle.hip: pack_cbhg)"""
    f = np.float64
    inv = (w[scope + '/gamma'].astype(f) if gamma else 1.0) / np.sqrt(w[scope + '/moving_variance'].astype(f) + BN_EPS)
    return inv.astype(np.float32), (w[scope + '/beta'].astype(f) - w[scope + '/moving_mean'].astype(f) * inv).astype(np.float32)


def check_stage(label, got, x, wt, ktaps, T, pool=0, bias=None, relu=False, scale=None, shift=None, resid=None, a=None):
    """got [M][N] against the float64 evaluation of ONE stage on x [M][Cin] (or on the operand rows `a` of a gather):
    prints phi of the GPU and of the model, holds the GPU to 4 x the model's.  Returns (phi GPU, phi model)."""
    f = np.float64
    a = G.im2col(x, ktaps, T, pool) if a is None else np.asarray(a, np.float32)
    N = wt.shape[0]
    acc = a.astype(f) @ wt.astype(f).T
    D = np.abs(a).astype(f) @ np.abs(wt).astype(f).T
    b = np.zeros(N, np.float32) if bias is None else np.asarray(bias, np.float32)
    sc = np.ones(N, np.float32) if scale is None else scale
    sh = np.zeros(N, np.float32) if shift is None else shift
    r = np.zeros_like(acc, dtype=np.float32) if resid is None else np.asarray(resid, np.float32)
    pre = acc + b.astype(f)
    ref = (np.maximum(pre, 0.0) if relu else pre) * sc.astype(f) + sh.astype(f) + r.astype(f)
    D = np.abs(sc).astype(f) * (D + np.abs(b).astype(f)) + np.abs(sh).astype(f) + np.abs(r).astype(f)
    Cin = a.shape[1] // ktaps
    m = G.model_products(a, wt, G.k_order(Cin, ktaps, pool), G.slice_tiles(a.shape[1]), [G.PAIRS])[0]
    m = m + b
    if relu:
        m = np.maximum(m, np.float32(0))
    m = ((m * sc + sh).astype(np.float32) + r).astype(np.float32)
    p_gpu, p_model = G.phi(got, ref, D), G.phi(m, ref, D)
    print('stage phi {}: GPU {:.3f} u, model {:.3f} u'.format(label, p_gpu, p_model))
    assert np.isfinite(np.asarray(got)).all()
    assert p_gpu <= BOUND_FACTOR * p_model, (label, p_gpu, p_model)
    return p_gpu, p_model


def check_front(label, ws, w, scope, hp, x, T):
    """bank / p1 / p2 of a CBHG from x [M][c_in] (what the kernels read) and the workspaces ws"""
    NB, NF = hp.n_banks, hp.n_filters
    for k in range(1, NB + 1):     # the grouped launch: widest first, written at channel offset (k - 1) NF
        cs = '{}/convolution_banks/conv-{}-{}'.format(scope, k, NF)
        sc, sh = fold_bn(w, '{}/convolution_banks/{}'.format(scope, _bn_name(k - 1)), gamma=False)
        check_stage('{} bank k={}'.format(label, k), ws['bank'][:, (k - 1) * NF:k * NF], x, G.weight_rows(w[cs + '/kernel']), k, T,
                    bias=w[cs + '/bias'], relu=True, scale=sc, shift=sh)
    (f1, k1, _), (f2, k2, _) = hp.projections
    ps = '{}/projections/1-conv-{}-{}'.format(scope, k1, f1)
    sc, sh = fold_bn(w, ps + '/batch_normalization', gamma=True)
    check_stage(label + ' p1', ws['p1'], ws['bank'], G.weight_rows(w[ps + '/conv1d/kernel']), k1, T, pool=1,
                bias=w[ps + '/conv1d/bias'], relu=True, scale=sc, shift=sh)
    ps = '{}/projections/2-conv-{}-{}'.format(scope, k2, f2)
    sc, sh = fold_bn(w, ps + '/batch_normalization', gamma=True)
    check_stage(label + ' p2', ws['p2'], ws['p1'], G.weight_rows(w[ps + '/conv1d/kernel']), k2, T,
                bias=w[ps + '/conv1d/bias'], scale=sc, shift=sh, resid=x)


def gru_projection(w, scope, U):
    """Wt [6H][U] and bias [6H] of the x-halves: [r | u | c] of fw, then of bw (csrc/api_handle.hip: pack_cbhg)"""
    rows, bias = [], []
    for d in ('fw', 'bw'):
        gs = '{}/gru/{}/gru_cell_{}'.format(scope, d, d)
        rows += [w[gs + '/gates/kernel'][:U].T, w[gs + '/candidate/kernel'][:U].T]
        bias += [w[gs + '/gates/bias'], w[gs + '/candidate/bias']]
    return np.ascontiguousarray(np.concatenate(rows, 0), dtype=np.float32), np.concatenate(bias).astype(np.float32)


def highway_weights(w, scope, n):
    out = []
    for l in range(n):
        hs = '{}/highway_network/highway_layer_{}'.format(scope, l)
        out.append((G.weight_rows(w[hs + '/H/kernel']), w[hs + '/H/bias'], G.weight_rows(w[hs + '/T/kernel']), w[hs + '/T/bias']))
    return out


def check_last_highway(label, x, y, layer):
    """One highway layer, y from x (hw1 -> hw0 of the layer-by-layer form): D = D_H + (|h+| + |x|) / 4 D_T + |h+| + |x|,
    D_H / D_T the sum |a||w| + |b| of the two halves, h+ = relu(H) (the sigmoid's slope is at most 1/4)."""
    f = np.float64
    wh, bh, wt, bt = layer
    x64 = x.astype(f)
    H = x64 @ wh.astype(f).T + bh.astype(f)
    Tt = x64 @ wt.astype(f).T + bt.astype(f)
    hp_, t = np.maximum(H, 0.0), 1.0 / (1.0 + np.exp(-Tt))
    ref = hp_ * t + x64 * (1.0 - t)
    D_H = np.abs(x64) @ np.abs(wh).astype(f).T + np.abs(bh).astype(f)
    D_T = np.abs(x64) @ np.abs(wt).astype(f).T + np.abs(bt).astype(f)
    D = D_H + (hp_ + np.abs(x64)) / 4 * D_T + hp_ + np.abs(x64)
    acc_h, = G.dense_model_many(x, wh, [G.PAIRS])
    acc_t, = G.dense_model_many(x, wt, [G.PAIRS])
    m = G.highway_epilogue32(acc_h, acc_t, bh, bt, x)
    p_gpu, p_model = G.phi(y, ref, D), G.phi(m, ref, D)
    print('stage phi {}: GPU {:.3f} u, model {:.3f} u'.format(label, p_gpu, p_model))
    assert p_gpu <= BOUND_FACTOR * p_model, (label, p_gpu, p_model)


def check_fused_stack(label, p2, hw0, lifter, layers, shape):
    """hw0 against the float64 chain from p2, per utterance, frame, channel and element; the tolerance is 4 x what the
    host chain (model GEMM + float32 epilogue per stage) reaches on the same input."""
    ref = G.tail_chain64(p2, lifter, layers).reshape(shape)
    host = G.tail_chain_model(p2, lifter, layers).reshape(shape)
    tol = BOUND_FACTOR * max(v[0] for v in slice_errors(host, ref, BTC).values())
    assert tol < 1e-5, tol
    assert_parity(hw0.reshape(shape), ref, BTC, tol, label)


def workspaces(eng, tag, M, c):
    ws = {k: eng.debug_workspace('{}.{}'.format(tag, k), (M, n)) for k, n in c.items()}
    return ws


def cbhg_dims(hp_part):
    U, H = hp_part.n_highway_units, hp_part.n_gru_units
    return {'bank': hp_part.n_banks * hp_part.n_filters, 'p1': hp_part.projections[0][0], 'p2': hp_part.projections[1][0],
            'hw0': U, 'hw1': U, 'xproj': 6 * H}


def check_tail(label, ws, w, scope, hp_part, fused, shape):
    """lifter / highway / GRU input projections from the workspaces of one run"""
    U = hp_part.n_highway_units
    lifter = (G.weight_rows(w[scope + '/lifter/kernel']), w[scope + '/lifter/bias'])
    layers = highway_weights(w, scope, hp_part.n_highway_layers)
    M = ws['p2'].shape[0]
    if hp_part.n_highway_layers == 0:
        check_stage(label + ' lifter', ws['hw0'], ws['p2'], lifter[0], 1, M, bias=lifter[1], relu=True)
    elif fused:
        check_fused_stack(label + ' highway stack', ws['p2'], ws['hw0'], lifter, layers, shape + (U,))
    elif hp_part.n_highway_layers % 2 == 0:     # ping-pong: the last layer read hw1, wrote hw0
        check_last_highway(label + ' last highway layer', ws['hw1'], ws['hw0'], layers[-1])
    wt, b = gru_projection(w, scope, U)
    check_stage(label + ' xproj', ws['xproj'], ws['hw0'], wt, 1, M, bias=b)


@pytest.fixture(params=[1, 0], ids=['fused', 'layers'])
def fused(request, engine):
    engine.set_option('fused_tail', request.param)
    yield request.param
    engine.set_option('fused_tail', 1)


def test_encoder_gemm_stages(engine, hparams, weights, fused):
    B, Ts = ENC_SHAPE
    M, V = B * Ts, hparams.vocabulary_size
    ids = make_ids(np.random.default_rng(41), B, Ts)
    ids[0, 3], ids[1, 0], ids[2, Ts - 1] = V, -1, V + 1000          # outside the table: a zero row
    d_ids = engine.to_device(ids)                                    # (device-resident ids are not screened by the wrapper)
    mem = engine.encoder_forward(d_ids).to_host()
    d_ids.free()
    enc = hparams.encoder
    u1, u2 = enc.pre_net_layers[0][0], enc.pre_net_layers[1][0]
    pre1 = engine.debug_workspace('enc.pre1', (M, u1))
    pre2 = engine.debug_workspace('enc.pre2', (M, u2))
    ws = workspaces(engine, 'enc', M, cbhg_dims(enc))
    flat = ids.reshape(-1)
    inside = (flat >= 0) & (flat < V)
    rows = np.where(inside[:, None], weights['encoder/embedding'][np.where(inside, flat, 0)], np.float32(0))
    s1, s2 = ('encoder/pre_net/{}-FC-{}'.format(i + 1, u) for i, u in enumerate((u1, u2)))
    check_stage('enc pre1 (gather)', pre1, None, G.weight_rows(weights[s1 + '/kernel']), 1, Ts, bias=weights[s1 + '/bias'], relu=True, a=rows)
    assert (~inside).sum() == 3
    assert np.array_equal(pre1[~inside], np.broadcast_to(np.maximum(weights[s1 + '/bias'], 0), (3, u1)))
    check_stage('enc pre2', pre2, pre1, G.weight_rows(weights[s2 + '/kernel']), 1, Ts, bias=weights[s2 + '/bias'], relu=True)
    check_front('enc', ws, weights, 'encoder', enc, pre2, Ts)
    check_tail('enc fused={}'.format(fused), ws, weights, 'encoder', enc, fused, (B, Ts))
    # the attention keys from the memory (no bias)
    engine.decoder_forward(mem, 2)
    A = hparams.decoder.n_attention_units
    keys = engine.debug_workspace('dec.keys', (M, A))
    check_stage('dec.keys', keys, mem.reshape(M, -1), G.weight_rows(weights['decoder2/memory_layer/kernel']), 1, Ts)


@pytest.mark.parametrize('B,T', POST_SHAPES)
def test_postnet_gemm_stages(engine, hparams, weights, fused, B, T):
    M = B * T
    mel = np.random.default_rng(300 + T).random((B, T, hparams.n_mels)).astype(np.float32)
    lin = engine.postnet_forward(mel).to_host()
    post = hparams.post
    ws = workspaces(engine, 'post', M, cbhg_dims(post))
    gru = engine.debug_workspace('post.gru', (M, 2 * post.n_gru_units))
    label = 'post T={}'.format(T)
    check_front(label, ws, weights, 'post_process', post, mel.reshape(M, -1), T)
    check_tail('{} fused={}'.format(label, fused), ws, weights, 'post_process', post, fused, (B, T))
    # the final Dense: N = 1025, one live column in the last tile
    check_stage(label + ' linear', lin.reshape(M, -1), gru, G.weight_rows(weights['dense/kernel']), 1, T, bias=weights['dense/bias'])


@pytest.mark.parametrize('fused_tail', [1, 0], ids=['fused', 'layers'])
def test_lifter_alone(hparams, fused_tail):
    """n_highway_layers = 0: hw0 is the lifter alone, relu(p2 W + b) -- 128 wide in the encoder, 80 wide (a padded k-chunk
    of the tail kernel) in the post-net, in both forms of the tail."""
    hp = copy.deepcopy(hparams)
    hp.encoder.n_highway_layers = 0
    hp.post.n_highway_layers = 0
    w = pkg('tacotron.weights').synthetic_weights(3, hp)
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        eng.set_option('fused_tail', fused_tail)
        B, Ts = ENC_SHAPE
        eng.encoder_forward(make_ids(np.random.default_rng(43), B, Ts))
        ws = workspaces(eng, 'enc', B * Ts, cbhg_dims(hp.encoder))
        check_tail('enc no highway fused={}'.format(fused_tail), ws, w, 'encoder', hp.encoder, fused_tail, (B, Ts))
        B, T = POST_SHAPES[0]
        eng.postnet_forward(np.random.default_rng(44).random((B, T, hp.n_mels)).astype(np.float32))
        ws = workspaces(eng, 'post', B * T, cbhg_dims(hp.post))
        check_tail('post no highway fused={}'.format(fused_tail), ws, w, 'post_process', hp.post, fused_tail, (B, T))
    finally:
        eng.close()


def test_more_banks_than_one_launch():
    """17 and 18 conv banks (tests/arch_cases.py 'wide'): a second grouped launch, kernels wider than 16 taps -- the
    loader's general path -- beside fast-path groups, split-K projections with K = 4896 / 8640."""
    hp, w, _ = arch_cases.arch('wide')
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        B, Ts = 2, 24
        M = B * Ts
        eng.encoder_forward(make_ids(np.random.default_rng(45), B, Ts))
        dims = {k: v for k, v in cbhg_dims(hp.encoder).items() if k in ('bank', 'p1', 'p2')}
        pre2 = eng.debug_workspace('enc.pre2', (M, hp.encoder.pre_net_layers[1][0]))
        check_front('wide enc', workspaces(eng, 'enc', M, dims), w, 'encoder', hp.encoder, pre2, Ts)
        B, T = 2, 20
        M = B * T
        mel = np.random.default_rng(46).random((B, T, hp.n_mels)).astype(np.float32)
        eng.postnet_forward(mel)
        dims = {k: v for k, v in cbhg_dims(hp.post).items() if k in ('bank', 'p1', 'p2')}
        check_front('wide post', workspaces(eng, 'post', M, dims), w, 'post_process', hp.post, mel.reshape(M, -1), T)
    finally:
        eng.close()
