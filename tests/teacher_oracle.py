"""Float64 numpy restatement of the teacher-forced decoder (reference tacotron/helpers.py:208-405, TacotronTrainingHelper,
chosen at tacotron/model.py:284-298) on the inference network of ``oracle.tacotron_oracle.decoder``, composed from that
module's primitives (a plain helper module, imported like conftest's helpers).

TacotronTrainingHelper feeds the GO frame (zeros) at step 0 and ``outputs[:, time]`` of ``outputs[:, r-1::r]`` -- target
frame t*r - 1 -- at step t >= 1; the last r-frame group of the target is never fed.  Everything else is Mode.PREDICT's
network: pre-net dropout off, no batch statistics, no gradient (this is not Mode.TRAIN)."""
import numpy as np

from oracle import tacotron_oracle as O


def teacher_inputs(mel_target, hp, n_steps):
    """(S, B, n_mels) decoder inputs: zeros at step 0, frame t*r - 1 of mel_target ((B, S, r*n_mels) or (B, S*r, n_mels))
    at step t >= 1."""
    B = mel_target.shape[0]
    frames = np.asarray(mel_target).reshape(B, n_steps * hp.reduction, hp.n_mels)
    x = np.zeros((n_steps, B, hp.n_mels), dtype=np.float64)
    for t in range(1, n_steps):
        x[t] = frames[:, t * hp.reduction - 1]
    return x


def decoder_teacher(memory, mel_target, w, hp):
    """The decoder loop of ``oracle.tacotron_oracle.decoder`` with the pre-net fed by :func:`teacher_inputs`.
    Returns (reduced_mel (B, S, r*n_mels), alignments (S, B, T_s)) with S = mel_target's r-frame groups."""
    dec = hp.decoder
    cudnn = bool(hp.force_cudnn)
    B, Ts, _ = memory.shape
    dt = memory.dtype
    S = int(np.prod(mel_target.shape)) // (B * hp.reduction * hp.n_mels)
    A, U = dec.n_attention_units, dec.n_decoder_gru_units
    att_hp = getattr(hp, 'attention', None)
    local = att_hp is not None and att_hp.mechanism == 'LocalLuongAttention'
    predictive = local and att_hp.luong_local_mode == 'predictive'
    keys = memory @ w['decoder2/memory_layer/kernel']
    xs = teacher_inputs(mel_target, hp, S).astype(dt)
    att = np.zeros((B, A), dtype=dt)
    h_att = np.zeros((B, A), dtype=dt)
    hs = [np.zeros((B, U), dtype=dt) for _ in range(dec.n_gru_layers)]
    outs = np.zeros((B, S, dec.target_size * hp.reduction), dtype=dt)
    aligns = np.zeros((S, B, Ts), dtype=dt)
    for t in range(S):
        p = O.pre_net(np.concatenate([xs[t], att], -1), w, O._ATT + '/pre_net', dec.pre_net_layers)
        h_att = O.gru_cell(p, h_att, w, O._ATT + '/gru_cell', cudnn)
        if predictive:
            ctx, a, _ = O.local_luong_predictive(h_att, keys, memory, w[O._ATT + '/local_luong_attention/local_w_p'],
                                                 w[O._ATT + '/local_luong_attention/local_v_p'],
                                                 att_hp.luong_local_window_D, att_hp.luong_force_gaussian)
        elif local:
            ctx, a = O.local_luong_monotonic(h_att, keys, memory, t, att_hp.luong_local_window_D,
                                             att_hp.luong_force_gaussian)
        else:
            a = O.softmax_lastaxis(np.einsum('bd,btd->bt', h_att, keys))
            ctx = np.einsum('bt,btd->bd', a, memory)
        att = np.concatenate([h_att, ctx], -1) @ w[O._ATT + '/attention_layer/kernel']
        y = att
        for i in range(dec.n_gru_layers):
            hs[i] = O.gru_cell(y, hs[i], w, '{}/cell_{}/gru_cell'.format(O._MRC, i + 1), cudnn)
            y = y + hs[i]
        outs[:, t] = y @ w['decoder2/decoder/output_projection_wrapper/kernel'] \
            + w['decoder2/decoder/output_projection_wrapper/bias']
        aligns[t] = a
    return outs, aligns


def teacher_forced(ids, mel_target, w, hp):
    """Encoder, :func:`decoder_teacher`, post-net (or the final Dense alone): (mel (B, T, n_mels), alignments, linear)."""
    B = ids.shape[0]
    memory = O.encoder(ids, w, hp)
    red, al = decoder_teacher(memory, mel_target, w, hp)
    mel = red.reshape(B, -1, hp.n_mels)
    lin = O.post_process(mel, w, hp) if hp.apply_post_processing else O.dense(mel, w, 'dense')
    return mel, al, lin
