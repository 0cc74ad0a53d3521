"""The architectures, shapes and inputs of the architecture tests (a plain helper module, imported like conftest's helpers).

tests/test_gpu_architectures.py runs the HIP network at every architecture of ARCHS against the float64 oracle;
tests/test_architectures_host.py shows on the CPU that the bounds it uses are fair on these very inputs (a float32 run of the
oracle stays within a quarter of each) and have teeth (a wrong restatement of the decoder misses them a hundredfold).  Both
draw architectures, weights and inputs from here, so that they cannot drift apart.

Every entry of ARCHS moves fields of the reference's model_params that tts_create accepts off their defaults and names the
code it is there for:

  narrow        1 conv bank, N = 4 / 16 / 32 GEMM columns, Cin = 16, a 5-entry embedding 16 wide, n_mels 16, r = 1 (the
                folded output projection is the WHOLE projection, the teacher stride is n_mels)
  wide          17 / 18 conv banks (a second bank launch; more than 16 taps: the GEMM loader's general path), split-K
                projections with K = 4896 / 8640, a CBHG tail input of 192 (> 128: layer by layer), n_mels 144 and r = 3
                in both persistent decoders, a 300-entry embedding 528 wide
  deep          4 decoder GRU layers, n_mels 272, decoder pre-net (528, 48): the second k pass of the launch-per-layer
                decoder GEMM in pre-net 1 (step 0: K = 272 + 256) and pre-net 2 (K = 528); outside both persistent kernels
  one, three    1 and 3 decoder GRU layers (the y0 / y1 ping-pong and the state layout), one of them with r = 7
  cudnn-narrow  n_mels 16, r = 2 with CudnnCompatibleGRUCell
  r1, r2        the reference architecture with r = 1 and r = 2 alone
"""
import copy
import functools
from collections import OrderedDict

import numpy as np

from conftest import pkg
from oracle import tacotron_oracle as O

# the bounds of the suite (tests/test_gpu_network.py, test_gpu_persistent.py, test_gpu_evaluate.py)
STAGE_TOL = 1e-4      # stage intermediates
FINAL_TOL = 1e-3      # memory, post-net bi-GRU output, mel, linear
ALIGN_TOL = 1e-4      # every alignment row
LOSS_TOL = 1e-5       # the three losses and the per-utterance sums, relative
HOST_MARGIN = 0.25    # float32 arithmetic itself stays within this fraction of every bound
TEETH = 100.0         # ... and a wrong restatement misses a bound by at least this factor


def _relu(*units):
    return tuple((u, 0.5, 'relu') for u in units)


def _proj(a, b):
    return ((a, 3, 'relu'), (b, 3, None))


def _narrow_post(hp):
    hp.post.n_banks, hp.post.n_filters, hp.post.projections = 1, 32, _proj(4, 16)


def _narrow(hp):
    hp.vocabulary_size, hp.n_mels, hp.reduction = 5, 16, 1
    hp.encoder.embedding_size = 16
    hp.encoder.pre_net_layers = _relu(32, 16)
    hp.encoder.n_banks, hp.encoder.n_filters, hp.encoder.projections = 1, 32, _proj(4, 16)
    _narrow_post(hp)


def _wide(hp):
    hp.vocabulary_size, hp.n_mels, hp.reduction = 300, 144, 3
    hp.encoder.embedding_size = 528
    hp.encoder.pre_net_layers = _relu(272, 192)
    hp.encoder.n_banks, hp.encoder.n_filters, hp.encoder.projections = 17, 96, _proj(100, 192)
    hp.post.n_banks, hp.post.n_filters, hp.post.projections = 18, 160, _proj(36, 144)


def _deep(hp):
    hp.n_mels, hp.reduction = 272, 2
    hp.decoder.n_gru_layers = 4
    hp.decoder.pre_net_layers = _relu(528, 48)
    hp.post.projections = _proj(256, 272)


def _one(hp):
    hp.decoder.n_gru_layers = 1
    hp.reduction = 7


def _three(hp):
    hp.decoder.n_gru_layers = 3


def _cudnn_narrow(hp):
    hp.n_mels, hp.reduction, hp.force_cudnn = 16, 2, True
    _narrow_post(hp)


def _r1(hp):
    hp.reduction = 1


def _r2(hp):
    hp.reduction = 2


ARCHS = OrderedDict([('narrow', _narrow), ('wide', _wide), ('deep', _deep), ('one', _one), ('three', _three),
                     ('cudnn-narrow', _cudnn_narrow), ('r1', _r1), ('r2', _r2)])

ENC_SHAPES = [(2, 7), (3, 37), (4, 24)]                 # Ts % 3 = 1, 1, 0 (the bi-GRU loop is unrolled by three)
POST_SHAPES = [(2, 15), (2, 20), (3, 100), (1, 1)]      # T % 3 = 0, 2, 1 and one frame; 300 rows = three tiles of the tail
DEC_SHAPES = [(2, 7, 3), (3, 37, 10), (17, 50, 6)]      # 17 utterances span two clusters of 16
# (persistent_decoder, pd_ws, pd_rows) and what tts_decoder_kernel_choice reports where the architecture admits the kernel
FORMS = OrderedDict([('launch-per-layer', ((0, 1, 0), 0)), ('weight-stationary-16', ((2, 1, 16), 2)),
                     ('weight-stationary-32', ((2, 1, 32), 2)), ('streamed-weights', ((2, 0, 0), 1))])


def configure(hparams, name):
    """A deep copy of the reference hyper-parameters with the architecture's fields moved; decoder.target_size follows n_mels."""
    hp = copy.deepcopy(hparams)
    ARCHS[name](hp)
    hp.decoder.target_size = hp.n_mels
    return hp


def seed_of(name):
    return 20 + list(ARCHS).index(name)


@functools.lru_cache(maxsize=None)
def arch(name):
    """(hp, float32 weights, float64 weights) of a named architecture; the weights are shared and never written."""
    hp = configure(pkg('tacotron.params').ModelParams(), name)
    w = pkg('tacotron.weights').synthetic_weights(seed_of(name), hp)
    return hp, w, O.cast_weights(w, np.float64)


def persistent_kernels(hp):
    """Which persistent decoder kernels cover the architecture (csrc: decoder_ws_supports, decoder_persistent_supports):
    two GRU layers and the reference's decoder pre-net for both; n_mels <= 256 (a multiple of 16 for the streamed form)."""
    ok = hp.decoder.n_gru_layers == 2 and tuple(l[0] for l in hp.decoder.pre_net_layers) == (256, 128) and hp.n_mels <= 256
    return {2: ok, 1: ok and hp.n_mels % 16 == 0, 0: True}


def expected_choice(hp, form):
    want = FORMS[form][1]
    return want if persistent_kernels(hp)[want] else 0


def expected_teacher_choice(hp, form):
    return 2 if expected_choice(hp, form) == 2 else 0


# ---------------------------------------------------------------------------------------------- inputs
def enc_ids(hp, B, Ts, seed=None):
    """Padded sentences from the architecture's own vocabulary: ids 2 .. V - 1, an EOS (1), zero padding."""
    rng = np.random.default_rng(100 + B if seed is None else seed)
    ids = rng.integers(2, hp.vocabulary_size, (B, Ts)).astype(np.int32)
    for b in range(B):
        L = int(rng.integers(max(2, Ts // 2), Ts))
        ids[b, L - 1] = 1
        ids[b, L:] = 0
    return ids


def with_unknown_ids(hp, ids):
    """One id just past the table and one far past it: they read as zero embedding rows (include/sstts_hip.h)."""
    out = ids.copy()
    out[0, 1] = hp.vocabulary_size
    out[-1, 2] = hp.vocabulary_size + 1000
    return out


def post_mel(hp, B, T):
    return np.random.default_rng(300 + B).random((B, T, hp.n_mels)).astype(np.float32)


def dec_memory(B, Ts):
    """A random memory scaled by 1.5 (tests/test_gpu_network.py::test_decoder): sharper attention than the encoder's own
    memory of random weights gives."""
    return (np.random.default_rng(200 + B).standard_normal((B, Ts, 256)) * 1.5).astype(np.float32)


def teacher_target(hp, B, S, seed=None):
    """normalised-dB-like mel targets (B, S, r * n_mels) in [0, 1)"""
    rng = np.random.default_rng(400 + B if seed is None else seed)
    return rng.random((B, S, hp.reduction * hp.n_mels)).astype(np.float32)


def net_shape(hp):
    """(B, Ts, S) of the whole-network tests: with r = 1 enough frames for Griffin-Lim's reflect padding (hop (T - 1) > n_fft / 2)."""
    return 3, 23, (8 if hp.reduction == 1 else 6)


def net_inputs(hp):
    B, Ts, S = net_shape(hp)
    F = 1 + hp.n_fft // 2
    ids = enc_ids(hp, B, Ts, seed=7)
    mel_t = teacher_target(hp, B, S, seed=8)
    lin_t = np.random.default_rng(9).random((B, S, hp.reduction * F)).astype(np.float32)
    for b in range(B):   # zero padding at the end of the shorter utterances, as the loader pads a batch
        keep = max(1, S * hp.reduction - 2 * b)
        mel_t.reshape(B, S * hp.reduction, -1)[b, keep:] = 0
        lin_t.reshape(B, S * hp.reduction, -1)[b, keep:] = 0
    return ids, mel_t, lin_t


# ---------------------------------------------------------------------------------------------- references
def encoder_ref(ids, w, hp):
    """(stages, memory) of the oracle's encoder; an id outside the table reads as a zero embedding row."""
    V = hp.vocabulary_size
    ids = np.asarray(ids)
    if (ids >= V).any():
        w = dict(w)
        emb = w['encoder/embedding']
        w['encoder/embedding'] = np.concatenate([emb, np.zeros((1, emb.shape[1]), emb.dtype)])
        ids = np.where(ids >= V, V, ids)
    stages = {}
    memory = O.encoder(ids, w, hp, stages)
    stages['proj2'] = stages['proj2'] + stages['prenet']   # what the "enc.p2" workspace holds: projection 2 + the residual
    return stages, memory


def postnet_ref(mel, w, hp):
    stages = {}
    linear = O.post_process(mel.astype(w['dense/kernel'].dtype), w, hp, stages)
    return stages, linear


def decoder_restated(memory, w, hp, n_steps, target=None, feed='last', top_residual=True):
    """The decoder loop of ``oracle.tacotron_oracle.decoder`` (target None) / ``teacher_oracle.decoder_teacher`` restated with
    two switches that make it WRONG on purpose: ``feed='first'`` feeds the first frame of the previous r-frame group instead
    of the last, ``top_residual=False`` drops the residual connection of the last decoder GRU layer.  Global Luong
    attention, both GRU formulations.  With the defaults it is the oracle, to the bit (tests/test_architectures_host.py)."""
    dec, r, NM = hp.decoder, hp.reduction, hp.n_mels
    cudnn = bool(hp.force_cudnn)
    B, Ts, _ = memory.shape
    dt = memory.dtype
    A, U = dec.n_attention_units, dec.n_decoder_gru_units
    keys = memory @ w['decoder2/memory_layer/kernel']
    frames = None if target is None else np.asarray(target, dtype=dt).reshape(B, n_steps * r, NM)
    x = np.zeros((B, NM), dtype=dt)
    att = np.zeros((B, A), dtype=dt)
    h_att = np.zeros((B, A), dtype=dt)
    hs = [np.zeros((B, U), dtype=dt) for _ in range(dec.n_gru_layers)]
    outs = np.zeros((B, n_steps, NM * r), dtype=dt)
    aligns = np.zeros((n_steps, B, Ts), dtype=dt)
    for t in range(n_steps):
        if frames is not None and t > 0:
            x = frames[:, t * r - 1] if feed == 'last' else frames[:, (t - 1) * r]
        p = O.pre_net(np.concatenate([x, att], -1), w, O._ATT + '/pre_net', dec.pre_net_layers)
        h_att = O.gru_cell(p, h_att, w, O._ATT + '/gru_cell', cudnn)
        a = O.softmax_lastaxis(np.einsum('bd,btd->bt', h_att, keys))
        ctx = np.einsum('bt,btd->bd', a, memory)
        att = np.concatenate([h_att, ctx], -1) @ w[O._ATT + '/attention_layer/kernel']
        y = att
        for i in range(dec.n_gru_layers):
            hs[i] = O.gru_cell(y, hs[i], w, '{}/cell_{}/gru_cell'.format(O._MRC, i + 1), cudnn)
            y = hs[i] if (i == dec.n_gru_layers - 1 and not top_residual) else y + hs[i]
        out = y @ w['decoder2/decoder/output_projection_wrapper/kernel'] + w['decoder2/decoder/output_projection_wrapper/bias']
        outs[:, t] = out
        aligns[t] = a
        x = out[:, -NM:] if feed == 'last' else out[:, :NM]
    return outs, aligns


def l1_sums(mel_t, lin_t, mel, lin):
    """Per-utterance sums (B, 2) = {sum |mel_t - mel|, sum |lin_t - lin|} and the three losses of Mode.EVAL, in float64."""
    B = mel.shape[0]
    d_mel = np.abs(mel_t.reshape(mel.shape).astype(np.float64) - mel)
    d_lin = np.abs(lin_t.reshape(lin.shape).astype(np.float64) - lin)
    sums = np.stack([d_mel.reshape(B, -1).sum(-1), d_lin.reshape(B, -1).sum(-1)], -1)
    dec, post = sums[:, 0].sum() / mel.size, sums[:, 1].sum() / lin.size
    return sums, np.array([dec + post, dec, post])


# ---------------------------------------------------------------------------------------------- cases: inputs + float64 references
# computed once per process and shared by the tests that need them (every decoder form of a shape, the host tests); read only
@functools.lru_cache(maxsize=None)
def encoder_case(name, B, Ts, unknown=False):
    hp, _, w64 = arch(name)
    ids = enc_ids(hp, B, Ts)
    if unknown:
        ids = with_unknown_ids(hp, ids)
    stages, memory = encoder_ref(ids, w64, hp)
    return ids, stages, memory


@functools.lru_cache(maxsize=None)
def postnet_case(name, B, T):
    hp, _, w64 = arch(name)
    mel = post_mel(hp, B, T)
    stages, linear = postnet_ref(mel, w64, hp)
    return mel, stages, linear


@functools.lru_cache(maxsize=None)
def decoder_case(name, B, Ts, S):
    hp, _, w64 = arch(name)
    memory = dec_memory(B, Ts)
    ref_mel, ref_al = O.decoder(memory.astype(np.float64), w64, hp, n_steps=S)
    return memory, ref_mel, ref_al


@functools.lru_cache(maxsize=None)
def teacher_case(name, B, Ts, S):
    import teacher_oracle as TO
    hp, _, w64 = arch(name)
    memory = dec_memory(B, Ts)
    target = teacher_target(hp, B, S)
    ref_mel, ref_al = TO.decoder_teacher(memory.astype(np.float64), target.astype(np.float64), w64, hp)
    return memory, target, ref_mel, ref_al


def network_ref(ids, mel_t, lin_t, w, hp):
    """Free-running and teacher-forced passes of the whole network with their per-utterance L1 sums and losses."""
    import teacher_oracle as TO
    dt = w['dense/kernel'].dtype
    free = O.tacotron_predict(ids, w, hp, n_steps=mel_t.shape[1])
    f_sums, f_losses = l1_sums(mel_t, lin_t, free['mel'], free['linear'])
    t_mel, t_al, t_lin = TO.teacher_forced(ids, mel_t.astype(dt), w, hp)
    t_sums, t_losses = l1_sums(mel_t, lin_t, t_mel, t_lin)
    return dict(memory=free['memory'], mel=free['mel'], alignments=free['alignments'], linear=free['linear'], sums=f_sums,
                losses=f_losses, t_mel=t_mel, t_alignments=t_al, t_linear=t_lin, t_sums=t_sums, t_losses=t_losses)


@functools.lru_cache(maxsize=None)
def network_case(name):
    hp, _, w64 = arch(name)
    ids, mel_t, lin_t = net_inputs(hp)
    return ids, mel_t, lin_t, network_ref(ids, mel_t, lin_t, w64, hp)
