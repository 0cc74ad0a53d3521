"""Host: the oracle of the estimated initial phases (tests/phase_oracle.py) against cases worked out by hand, its ownership
rules, ragged batches, the quality statement on the float64 Griffin-Lim oracle, and the surface of the feature that needs no
device: refusals of the library and ValueErrors of the Python layers."""
import ctypes

import numpy as np
import pytest

import momentum_oracle as M
import phase_cases as K
import phase_oracle as P
from conftest import pkg
from host_checks import no_device_engine

HALF = np.uint32(0x80000000)


# ---------------------------------------------------------------------------------------------- the oracle by hand
def _one_peak(F, j, T, left, right):
    m = np.zeros((F, T), np.float32)
    m[j] = 4.0
    m[j - 1] = left
    m[j + 1] = right
    return m


def test_a_stationary_peak_keeps_its_phase_and_its_lobe_alternates():
    # n_fft 256, hop 64, peak at bin 8 with equal neighbours: p = 0, x = 64 * 8 / 256 = 2, adv = 0
    assert P.peak_advance(1.0, 4.0, 1.0, 8, 64, 256) == 0
    phi = P.phase_track(_one_peak(129, 8, 6, 1.0, 1.0), 256, 64)
    assert not phi[8].any()
    # bins 7 and 9 are owned by the peak: half a turn off; everything else is a tie without an owner
    assert (phi[7] == HALF).all() and (phi[9] == HALF).all()
    assert not np.delete(phi, [7, 9], axis=0).any()
    u = P.phase_estimate(_one_peak(129, 8, 6, 1.0, 1.0), 256, 64)
    assert u.dtype == np.float32 and (u[7] == 0.5).all() and (u[9] == 0.5).all() and (u[8] == 0.0).all()
    # a wider lobe alternates 0 / 0.5 bin by bin
    m = np.zeros((129, 4), np.float32)
    m[5:12] = np.array([1, 2, 3, 4, 3, 2, 1], np.float32)[:, None]
    u = P.phase_estimate(m, 256, 64)
    assert (u[4:13, :] == np.array([0.0, 0.5, 0.0, 0.5, 0.0, 0.5, 0.0, 0.5, 0.0], np.float32)[:, None]).all()


def test_a_peak_between_two_hops_advances_by_a_quarter_turn_exactly():
    # peak at bin 9: x = 64 * 9 / 256 = 2.25, adv = 2^30 per frame
    assert P.peak_advance(1.0, 4.0, 1.0, 9, 64, 256) == 1 << 30
    phi = P.phase_track(_one_peak(129, 9, 9, 1.0, 1.0), 256, 64)
    want = (np.arange(1, 10, dtype=np.uint64) << np.uint64(30)) & np.uint64(0xFFFFFFFF)
    assert (phi[9] == want.astype(np.uint32)).all()                 # wraps after four frames
    assert (phi[8] == phi[9] + HALF).all() and (phi[10] == phi[9] + HALF).all()
    u = P.phase_estimate(_one_peak(129, 9, 9, 1.0, 1.0), 256, 64)
    assert u[9].tolist() == [0.25, 0.5, 0.75, 0.0, 0.25, 0.5, 0.75, 0.0, 0.25]


def test_the_parabola_moves_the_frequency_off_the_bin():
    # neighbours 1 and 2 around 4: p = 0.5 (1 - 2) / ((1 - 8) + 2) = 0.1, x = 64 * 8.1 / 256 = 2.025
    a, b, g = np.float64(1.0), np.float64(4.0), np.float64(2.0)
    p = np.float64(0.5) * (a - g) / ((a - np.float64(2.0) * b) + g)
    x = (np.float64(64) * (np.float64(8) + p)) / np.float64(256)
    assert P.peak_advance(1.0, 4.0, 2.0, 8, 64, 256) == int(np.floor((x - np.floor(x)) * 4294967296.0))
    assert abs(P.peak_advance(1.0, 4.0, 2.0, 8, 64, 256) / 2.0 ** 32 - 0.025) < 1e-9


# ---------------------------------------------------------------------------------------------- ownership
def _owners(values):
    return P.frame_owners(np.array(values, np.float32))


def test_ownership_rules():
    nan, inf = np.nan, np.inf
    #              0  1  2  3  4  5  6  7  8
    peak, own = _owners([0, 1, 3, 2, 1, 2, 5, 1, 0])
    assert np.flatnonzero(peak).tolist() == [2, 6]
    # bin 4 is a strict trough: the right-hand peak wins; bin 3 walks right into the trough? no: 2 > 1 stops it at once, so left
    assert own.tolist() == [2, 2, -1, 2, 6, 6, -1, 6, 6]
    # ties end walks: the plateau 3 3 is no peak and owns nothing; its slopes find no owner on that side
    peak, own = _owners([0, 1, 3, 3, 1, 0])
    assert not peak.any() and (own == -1).all()
    # a walk that ends at an edge finds no owner: a ramp to the last bin, a ramp from the first
    peak, own = _owners([0, 1, 2, 3, 4])
    assert not peak.any() and (own == -1).all()
    peak, own = _owners([4, 3, 2, 1, 0])
    assert not peak.any() and (own == -1).all()
    # ... but a ramp that turns one bin before the edge has a peak that owns the whole ramp
    peak, own = _owners([0, 1, 2, 3, 4, 0])
    assert np.flatnonzero(peak).tolist() == [4] and own.tolist() == [4, 4, 4, 4, -1, 4]
    # a NaN bin is no peak and ends every walk; its neighbours are no peaks either (the comparison with it is false)
    peak, own = _owners([0, 1, nan, 3, 5, 3, 1])
    assert np.flatnonzero(peak).tolist() == [4] and own.tolist() == [-1, -1, -1, 4, -1, 4, 4]
    peak, own = _owners([0, 2, 5, nan, 1, 0])
    assert not peak.any() and (own == -1).all()
    # +Inf is an ordinary large value; two of them side by side are a tie
    peak, own = _owners([0, 1, inf, 1, 0, inf, inf, 0])
    assert np.flatnonzero(peak).tolist() == [2] and own.tolist() == [2, 2, -1, 2, 2, -1, -1, -1]
    assert P.peak_advance(1.0, inf, 1.0, 8, 64, 256) == 0          # p = -0 or +0: the bin's own frequency
    assert P.peak_advance(-inf, 1.0, 0.5, 8, 64, 256) == 0         # fr is NaN: no advance


def test_all_zero_input_gives_all_zero_phases():
    for n_fft in (256, 2048):
        u = P.phase_estimate(np.zeros((1 + n_fft // 2, 5), np.float32), n_fft, K.HOP[n_fft])
        assert u.shape == (1 + n_fft // 2, 5) and not u.any() and not np.signbit(u).any()


def test_an_unowned_bin_keeps_its_phase_from_frame_to_frame():
    m = np.zeros((129, 3), np.float32)
    m[:, 0] = _one_peak(129, 9, 1, 1.0, 1.0)[:, 0]      # frame 0: a peak at 9 that owns 8 and 10
    m[:, 2] = m[:, 0]                                    # frame 1 is flat: everything is kept
    phi = P.phase_track(m, 256, 64)
    assert phi[9].tolist() == [1 << 30, 1 << 30, 1 << 31]
    assert phi[8].tolist() == [3 << 30, 3 << 30, 0] and phi[10].tolist() == phi[8].tolist()


def test_ragged_batches_in_the_oracle():
    mag, n = K.ragged_batch(256, 11)
    got = P.phase_estimate(mag, 256, 64, n_frames=n, fill=-7.0)
    for b in range(3):
        alone = P.phase_estimate(np.ascontiguousarray(mag[b, :, :n[b]]), 256, 64)
        assert np.isfinite(alone).all()                  # the NaN behind the end was never read
        assert np.array_equal(got[b, :, :n[b]], alone) and (got[b, :, n[b]:] == -7.0).all()
    # the public value is exact, in [0, 1), a multiple of 2^-24
    u = P.phase_estimate(K.magnitudes('random', 256, 41), 256, 64)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * 2.0 ** 24, np.round(u * 2.0 ** 24))


# ---------------------------------------------------------------------------------------------- quality
def test_the_estimate_reaches_in_20_iterations_what_random_phases_reach_in_60():
    """float64 Griffin-Lim oracle, frames 100:260 of the shipped spectrogram.  Measured: 9.40e-6 after 20 iterations from the
    estimate against 1.341e-5 after 60 from default_rng(0) phases; 3.94e-5 against 4.21e-4 after the first."""
    mag, init = M.shipped_spectrogram(100, 260)
    est = P.phase_estimate(mag, 2048, 275)
    h_rand, h_est = [], []
    M.griffin_lim_momentum(mag, 1102, 275, 2048, 60, init, 0.0, history=h_rand)
    M.griffin_lim_momentum(mag, 1102, 275, 2048, 20, est, 0.0, history=h_est)
    print('random: 1 {:.3e}, 20 {:.3e}, 60 {:.3e};  estimate: 1 {:.3e}, 20 {:.3e}'.format(h_rand[0], h_rand[19], h_rand[59], h_est[0], h_est[19]))
    assert h_est[19] <= h_rand[59]
    assert h_est[0] < 0.25 * h_rand[0]


# ---------------------------------------------------------------------------------------------- the surface
def test_the_library_refuses_without_a_device():
    H = pkg('_hip')
    lib = H.load_library()
    assert 'tts_phase_estimate' in H.exported_symbols() and 'tts_phase_estimate_rows' in H.exported_symbols()
    assert lib.tts_phase_estimate(None, None, 1, 1, None, 2048, 275, None) == H.TTS_ERR_INVALID
    assert lib.tts_phase_estimate_rows(None, None, 1, 1, 1056, None, 2048, 275, None) == H.TTS_ERR_INVALID
    assert lib.tts_set_option(None, b'gl_init', 1) == H.TTS_ERR_INVALID
    assert lib.tts_phase_chunk_frames() >= 1


def test_phase_init_values():
    H = pkg('_hip')
    assert H.phase_init_value(None) is None and H.phase_init_value('random') == 0 and H.phase_init_value('estimate') == 1


@pytest.mark.parametrize('bad', ['Estimate', 'spsi', '', 1, 0, True, 1.0, b'estimate'])
def test_python_refuses_bad_phase_init_before_any_device_call(bad, tmp_path):
    H = pkg('_hip')
    I = pkg('tacotron.inference')   # noqa: E741
    V = pkg('tacotron.serve')
    Y = pkg('audio.synthesis')
    eng = no_device_engine()
    ids = np.ones((2, 5), np.int32)
    mag = np.ones((1, 1025, 12), np.float32)
    with pytest.raises(ValueError):
        H.phase_init_value(bad)
    with pytest.raises(ValueError):
        eng.griffin_lim(mag, 2, 1102, 275, 2048, phase_init=bad)
    with pytest.raises(ValueError):
        eng.synthesize(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, phase_init=bad)
    with pytest.raises(ValueError):
        eng.synthesize_host(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, phase_init=bad)
    with pytest.raises(ValueError):
        Y.griffin_lim_v2(mag[0], 1102, 275, 2048, 2, engine=eng, phase_init=bad)
    with pytest.raises(ValueError):
        Y.spectrogram_to_wav(mag[0], 1102, 275, 2048, 2, engine=eng, phase_init=bad)
    with pytest.raises(ValueError):
        I.synthesize_batch(None, ids, phase_init=bad)
    with pytest.raises(ValueError):
        next(I.synthesize_stream(None, [ids], phase_init=bad))
    with pytest.raises(ValueError):
        next(I.inference_stream(None, [ids], phase_init=bad))
    with pytest.raises(ValueError):
        I.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', phase_init=bad)
    with pytest.raises(ValueError):
        next(V.serve(iter([['x']]), '/nonexistent/weights', phase_init=bad))
    with pytest.raises(ValueError):
        V.post_process_spectrograms(np.zeros((1, 40, 1025), np.float32), None, phase_init=bad)


def test_python_refuses_bad_estimate_arguments_before_any_device_call():
    eng = no_device_engine()
    mag = np.ones((3, 129, 10), np.float32)
    for n_fft, hop in [(250, 64), (128, 32), (8192, 64), (256.5, 64), (256, 0), (256, 257), (256, 1.5), (512, 64)]:
        with pytest.raises(ValueError):
            eng.phase_estimate(mag, n_fft, hop)
    for bad in [[10, 7], [[10, 7, 1]], 10, [10, 0, 1], [10, 11, 1], [10.0, 7.0, 1.0]]:
        with pytest.raises(ValueError):
            eng.phase_estimate(mag, 256, 64, n_frames=bad)
    with pytest.raises(ValueError):
        eng.phase_estimate(np.ones((129, 10), np.float32), 256, 64)
    with pytest.raises(ValueError):
        eng.phase_estimate_rows(np.ones((3, 10, 129), np.float32), 256, 64, row_stride=128)
    with pytest.raises(ValueError):
        eng.phase_estimate_rows(np.ones((3, 129, 10), np.float32), 256, 64)     # (B, F, T) is not time-major


def test_command_line_parses_and_checks_the_start(tmp_path):
    I = pkg('tacotron.inference')   # noqa: E741
    assert I.parse_args([]).phase_init == 'random'
    assert I.parse_args(['--phase-init', 'estimate']).phase_init == 'estimate'
    # main() checks the value before it looks at a folder, a sentence file or a checkpoint
    with pytest.raises(ValueError, match='phase_init'):
        I.main(['--phase-init', 'spsi', '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])
    with pytest.raises(NotADirectoryError):   # a legal value gets as far as the reference's first check
        I.main(['--phase-init', 'estimate', '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])


def test_the_cases_are_what_they_say():
    """the inputs of the GPU tests exercise what they are named for (checked on the oracle, once, at the small size)"""
    F, T = 129, 6
    up = P.frame_owners(K.magnitudes('ramp-up', 256, T)[:, 0])
    assert np.flatnonzero(up[0]).tolist() == [F - 2] and (up[1][:F - 2] == F - 2).all()
    down = P.frame_owners(K.magnitudes('ramp-down', 256, T)[:, 0])
    assert np.flatnonzero(down[0]).tolist() == [1] and (down[1][2:] == 1).all()
    q = K.magnitudes('quantised', 256, T)
    assert (q[1:] == q[:-1]).mean() > 0.15
    c = K.magnitudes('chirp', 256, T)
    assert len({int(np.argmax(c[:, t])) for t in range(T)}) == T
    z = K.magnitudes('nan-inf', 256, T)
    assert np.isnan(z).any() and np.isinf(z).any()
    assert K.frame_counts(2048, 32) == [9, 31, 32, 33, 67] and K.frame_counts(2048, 16) == [9, 15, 16, 17, 31, 32, 33, 35, 67]
    assert ctypes.sizeof(ctypes.c_float) == 4
