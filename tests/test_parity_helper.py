"""CPU: the per-slice checks of tests/parity.py catch what one whole-tensor rel-L2 misses.

Faults of the shape the kernels' partitions would produce -- one utterance of a cluster, one GEMM column of an N-tile tail,
the last frame of a time tile, a little alignment mass moved inside one row -- are planted in float64 oracle outputs.  Each
passes the whole-tensor check the GPU tests have always made and fails the per-slice one they make now; an unperturbed
float32 copy passes both, and all-zero padded frames do not trip the floor."""
import numpy as np
import pytest

from conftest import rel_l2
from oracle import tacotron_oracle as O
from parity import (BTC, alignment_rows, assert_alignment_rows, assert_mel_parity, assert_parity, assert_segment_parity,
                    slice_errors)

FINAL_TOL = 1e-3


@pytest.fixture(scope='module')
def decoder_ref(hparams, weights64):
    """The oracle's decoder at B = 80 (five 16-row clusters), Ts = 33, S = 3."""
    rng = np.random.default_rng(280)
    memory = rng.standard_normal((80, 33, 256)) * 1.5
    mel, al = O.decoder(memory, weights64, hparams, n_steps=3)
    assert mel.shape == (80, 3, 400) and al.shape == (3, 80, 33)
    return mel, al


@pytest.fixture(scope='module')
def linear_ref(hparams, weights64):
    """The oracle's post-net on a small random mel: [2, 100, 1025]."""
    mel = np.random.default_rng(281).random((2, 100, 80))
    lin = O.post_process(mel, weights64, hparams)
    assert lin.shape == (2, 100, 1025)
    return lin


def _fails(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_unperturbed_float32_copies_pass(decoder_ref, linear_ref):
    mel, al = decoder_ref
    assert_mel_parity(mel.astype(np.float32), mel, FINAL_TOL, 'clean')
    assert_alignment_rows(al.astype(np.float32), al, 1e-4, 'clean')
    assert_parity(linear_ref.astype(np.float32), linear_ref, BTC, FINAL_TOL, 'clean linear')
    e = slice_errors(mel, mel, BTC)
    assert all(v[0] == 0.0 for v in e.values())


def test_one_utterance_of_eighty(decoder_ref):
    """The last row of the tail cluster 1 + 6e-3 off: 6e-3 / sqrt(80) = 6.7e-4 in the whole tensor."""
    mel, _ = decoder_ref
    bad = mel.copy()
    bad[79] *= 1 + 6e-3
    assert 4e-4 < rel_l2(bad, mel) < FINAL_TOL
    _fails(assert_mel_parity, bad, mel, FINAL_TOL, 'planted utterance')
    e = slice_errors(bad, mel, {'utt': 0})
    assert e['utt'][1] == 79 and e['utt'][0] > 5e-3


def test_one_mel_column_of_four_hundred(decoder_ref):
    """One of the 400 reduced-mel GEMM columns offset by 1.5 % of its RMS: 1.5e-2 / sqrt(400) = 7.5e-4 in the whole tensor."""
    mel, _ = decoder_ref
    bad = mel.copy()
    col = 397
    bad[:, :, col] += 0.015 * np.sqrt(np.mean(mel[:, :, col] ** 2))
    assert 5e-4 < rel_l2(bad, mel) < FINAL_TOL
    _fails(assert_mel_parity, bad, mel, FINAL_TOL, 'planted column')
    e = slice_errors(bad, mel, {'col': 2})
    assert e['col'][1] == col and e['col'][0] > FINAL_TOL


def test_last_frame_of_a_linear_spectrogram(linear_ref):
    """The last of T = 100 frames 0.5 % off: 5e-3 / sqrt(100) = 5e-4 in the whole tensor."""
    bad = linear_ref.copy()
    bad[:, -1] *= 1 + 5e-3
    assert 3e-4 < rel_l2(bad, linear_ref) < FINAL_TOL
    _fails(assert_parity, bad, linear_ref, BTC, FINAL_TOL, 'planted frame')
    e = slice_errors(bad, linear_ref, BTC)
    assert e['frame'][1] == 99 and e['frame'][0] > FINAL_TOL


def test_one_gemm_column_in_an_n_tile_tail():
    """M = 150, N = 1025 (8 full N tiles + one column): that tail column 1 + 1e-4 off passes the GEMM tests' 1e-5."""
    rng = np.random.default_rng(1025)
    x = rng.standard_normal((150, 128))
    w = rng.standard_normal((1025, 128)) * 0.05
    ref = x @ w.T
    assert_parity(ref.astype(np.float32), ref, {'row': 0, 'col': 1}, 1e-5, 'clean gemm')
    bad = ref.copy()
    bad[:, 1024] *= 1 + 1e-4
    assert rel_l2(bad, ref) < 1e-5
    _fails(assert_parity, bad, ref, {'row': 0, 'col': 1}, 1e-5, 'planted gemm column')
    assert slice_errors(bad, ref, {'col': 1})['col'][1] == 1024


def test_alignment_mass_moved_inside_one_row(decoder_ref):
    """5e-5 of weight moved between two positions of one Ts = 33 row: the max-abs bound (1e-4) passes it, the row's rel-L2
    (about 4e-4 for a diffuse row) does not."""
    _, al = decoder_ref
    norms = np.linalg.norm(al, axis=-1)
    s, b = np.unravel_index(int(np.argmin(norms)), norms.shape)      # the most diffuse row
    bad = al.copy()
    bad[s, b, 3] += 5e-5
    bad[s, b, 20] -= 5e-5
    assert np.abs(bad - al).max() < 1e-4
    assert np.allclose(bad.sum(-1), 1.0)
    rows = alignment_rows(bad, al)
    assert rows[s, b] > 2e-4 and np.count_nonzero(rows) == 1
    _fails(assert_alignment_rows, bad, al, 1e-4, 'planted alignment')


def test_all_zero_padded_frames_do_not_trip_the_floor(linear_ref):
    """Frames whose reference is exactly zero (padding) are measured against the RMS frame norm, not against zero: float32
    rounding of the real frames and noise at 1e-7 of the RMS in the padded ones pass."""
    ref = linear_ref.copy()
    ref[:, 70:] = 0.0
    got = ref.astype(np.float32).astype(np.float64)
    rms_frame = np.linalg.norm(ref) / np.sqrt(ref.shape[1])
    got[:, 70:] = np.random.default_rng(0).standard_normal(got[:, 70:].shape) * 1e-7 * rms_frame / np.sqrt(1025)
    errs = assert_parity(got, ref, BTC, FINAL_TOL, 'padded linear')
    assert errs['frame'][0] < 1e-5
    # ... while a padded frame that is not zero on the device is still caught
    got[1, 85] += 0.01 * rms_frame / np.sqrt(1025)
    _fails(assert_parity, got, ref, BTC, FINAL_TOL, 'padded linear, dirty frame')


def _predictive_hp(hparams, D, vp_scale):
    import copy
    from conftest import pkg
    hp = copy.deepcopy(hparams)
    hp.attention.mechanism = 'LocalLuongAttention'
    hp.attention.luong_local_mode = 'predictive'
    hp.attention.luong_local_window_D = D
    hp.attention.luong_force_gaussian = True
    w = pkg('tacotron.weights').synthetic_weights(11, hp)
    vp = 'decoder2/decoder/output_projection_wrapper/multi_rnn_cell/cell_0/attention_wrapper/local_luong_attention/local_v_p'
    w[vp] = (w[vp] * vp_scale).astype(np.float32)
    return hp, w


def _centre_as_the_kernels_evaluate_it(query, w_p, v_p, Ts):
    """csrc/tts_common.h, predicted_centre: q W_p and the v_p reduction in double, tanh in float, the sigmoid's
    exponential in float with a first-order correction, the division in double, p rounded to float once."""
    qw = (query.astype(np.float64) @ w_p.astype(np.float64)).astype(np.float32)
    z = (np.tanh(qw).astype(np.float64) @ v_p.astype(np.float64))[:, 0]
    zf = z.astype(np.float32)
    e = np.exp(-zf).astype(np.float64) * (1.0 - (z - zf.astype(np.float64)))
    return (Ts / (1.0 + e)).astype(np.float32)


@pytest.mark.parametrize('B,Ts,S,D,vp_scale', [(3, 60, 12, 10, 1.0), (2, 150, 9, 10, 8.0)])
def test_predictive_gaussian_rows_need_an_accurate_centre(hparams, B, Ts, S, D, vp_scale, monkeypatch):
    """The predictive gaussian cases of tests/test_gpu_local_attention.py, restated in float32.  A reported weight is
    softmax * exp(-(j - p)^2 / 2 * (D/2)^2): it moves by (D/2)^2 (j - p) relative per unit of p, and float32 resolves
    p ~ 100 to 7.6e-6.  With p evaluated in float32 throughout, the worst alignment row at v_p x 8 misses the 1e-4 bound
    (so did every GPU decoder form with the fast float intrinsics, by 2-2.5x); with p evaluated as the kernels now do,
    only the float32 decoder state is left, and every row is inside the bound."""
    hp, w = _predictive_hp(hparams, D, vp_scale)
    memory = np.random.default_rng(7 * B + D).standard_normal((B, Ts, 256)).astype(np.float32) * 0.5
    _, ref_al = O.decoder(memory.astype(np.float64), O.cast_weights(w, np.float64), hp, n_steps=S)
    w32 = O.cast_weights(w, np.float32)
    _, al32 = O.decoder(memory, w32, hp, n_steps=S)
    plain = float(alignment_rows(al32, ref_al).max())

    orig, sigmoid = O.local_luong_predictive, O.sigmoid

    def with_kernel_centre(query, keys, values, w_p, v_p, d, force_gaussian):
        p = _centre_as_the_kernels_evaluate_it(query, w_p, v_p, keys.shape[1])
        # the oracle forms p = Ts * sigmoid(.): hand it p / Ts in float64 for this one call, so that it carries p itself
        monkeypatch.setattr(O, 'sigmoid', lambda x: p[:, None].astype(np.float64) / keys.shape[1])
        try:
            out = orig(query, keys, values, w_p, v_p, d, force_gaussian)
        finally:
            monkeypatch.setattr(O, 'sigmoid', sigmoid)
        np.testing.assert_allclose(out[2], p, rtol=1e-14, atol=0)
        return out

    monkeypatch.setattr(O, 'local_luong_predictive', with_kernel_centre)
    _, al_k = O.decoder(memory, w32, hp, n_steps=S)
    accurate = float(alignment_rows(al_k, ref_al).max())
    print('predictive gaussian B={} Ts={} v_p x {}: worst alignment row, float32 restatement {:.3e}, with the kernels\' '
          'centre {:.3e}'.format(B, Ts, vp_scale, plain, accurate))
    assert accurate < 1e-4
    if vp_scale == 8.0:
        assert plain > 1e-4


def test_one_hop_segment_of_a_waveform():
    """a 1e-3 error in the LAST hop segment of 150 (the halo / window-sum edge of an utterance) moves the utterance's
    rel-L2 by 8e-5 and passes 1e-4; the per-segment check fails it, for one waveform and for a batch"""
    rng = np.random.default_rng(5)
    hop, T = 275, 151
    ref = rng.standard_normal((3, hop * (T - 1)))
    got = ref.astype(np.float32).astype(np.float64)
    assert_segment_parity(got, ref, hop, 1e-4, 'clean batch')
    assert_segment_parity(got[1], ref[1], hop, 1e-4, 'clean')
    got[1, -hop:] *= 1.001
    assert rel_l2(got[1], ref[1]) < 1e-4
    for g, r in ((got[1], ref[1]), (got, ref)):
        with pytest.raises(AssertionError) as e:
            assert_segment_parity(g, r, hop, 1e-4, 'last segment')
        assert 'seg' in str(e.value) and str(T - 2) in str(e.value)
    assert_segment_parity(got[0], ref[0], hop, 1e-4, 'the other utterances')
