"""Speaking rate without a GPU: the oracle (tests/stretch_oracle.py) held to itself -- the round-once blend the library
computes against the whole phase-vocoder path of the reference's time_stretch (audio/effects.py:46-88), on the arrays the GPU
tests use -- the frame count of the library and of the Python surface against np.arange, and every Python refusal, raised before
a handle, a model or a device is touched."""
import ctypes

import numpy as np
import pytest

import stretch_cases as K
import stretch_oracle as S
from conftest import pkg
from host_checks import no_device_engine

# the issue's bar: four times the derived 2^-22 (complex64 cast 2^-24, float32 abs 2^-23, the blend's own rounding 2^-24)
FULL_PATH_TOL = 1e-6


def test_frame_counts_are_np_arange():
    H = pkg('_hip')
    lib = H.load_library()
    for r in sorted(set(K.HOST_RATES + K.STAGE_RATES + [0.25, 4.0])):
        for n in range(1, 65):
            want = len(np.arange(0, n, r))
            assert S.stretched_frames(n, r) == want
            assert H.stretched_frames(n, r) == want, (n, r)
            out = ctypes.c_int(-1)
            assert lib.tts_stretched_frames(n, r, ctypes.byref(out)) == H.TTS_OK and out.value == want, (n, r)
    out = ctypes.c_int(-1)
    for n, r in [(0, 1.0), (-1, 1.0), (5, float('nan')), (5, float('inf')), (5, 0.0), (5, 0.2), (5, 4.5)]:
        assert lib.tts_stretched_frames(n, r, ctypes.byref(out)) == H.TTS_ERR_INVALID and out.value == -1, (n, r)
    assert lib.tts_stretched_frames(5, 1.0, None) == H.TTS_ERR_INVALID


def _hold_to_full_path(mag, phase, rate, label):
    got = S.blend(mag, rate)
    full = S.vocoder_abs(mag, phase, rate)
    assert got.shape == full.shape == (mag.shape[0], S.stretched_frames(mag.shape[1], rate)), label
    zero = full == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()), np.float32)), label   # where the reference gives zero: exactly zero
    err = np.abs(got.astype(np.float64) - full.astype(np.float64))[~zero] / full.astype(np.float64)[~zero]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= FULL_PATH_TOL, (label, worst)
    return worst


def test_round_once_blend_against_the_full_phase_vocoder_path():
    """random magnitudes, F = 129, T in {1, 7, 12, 25, 40}: the counts and steps are np.arange's, the blend is the whole path's
    np.abs to rounding"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for T in K.HOST_T:
        mag = rng.random((129, T)).astype(np.float32)
        phase = rng.uniform(-np.pi, np.pi, (129, T))
        for r in K.HOST_RATES:
            assert np.array_equal(S.time_steps(T, r), np.arange(0, T, r, dtype=float))
            worst = max(worst, _hold_to_full_path(mag, phase, r, (T, r)))
    print('worst relative difference {:.3e} (derived bound 2^-22 = {:.3e})'.format(worst, S.BOUND_FULL_PATH))
    assert worst <= S.BOUND_FULL_PATH * 1.0000001


@pytest.mark.parametrize('F', K.STAGE_F)
def test_the_gpu_tests_inputs_against_the_full_path(F):
    x, ph = K.stage_batch(F), K.stage_phases(F)
    for r in K.STAGE_RATES:
        for b, n in enumerate(K.STAGE_LENGTHS):
            _hold_to_full_path(x[b, :, :n], ph[b, :, :n], r, (F, r, b, n))
            _hold_to_full_path(x[b], ph[b], r, (F, r, b, 'all'))


def test_oracle_batch_form_and_rate_one():
    x = K.stage_batch(129)
    assert np.array_equal(S.blend_batch(x, 1.0).view(np.uint32), x.view(np.uint32))      # rate 1.0: the input bits
    y = S.blend_batch(K.poisoned(x, K.STAGE_LENGTHS), 1.3, K.STAGE_LENGTHS, T_out=13)
    assert y.shape == (3, 129, 13) and not np.isnan(y).any()                             # nothing behind a length is read
    for b, n in enumerate(K.STAGE_LENGTHS):
        m = S.stretched_frames(n, 1.3)
        assert not y[b, :, m:].any() and np.array_equal(y[b, :, :m], S.blend(x[b, :, :n], 1.3))
    # the last frame of an utterance blends with the zero padding: (1 - a) x[n - 1]
    one = S.blend(np.array([[2.0]], np.float32), 0.5)
    assert one.tolist() == [[2.0, 1.0]]
    # 0 * NaN stays NaN (rate 2.0 reads x[1] with a == 0 through x[0]'s frame: i = 0, a = 0, neighbour x[1])
    assert np.isnan(S.blend(np.array([[1.0, np.nan, 3.0, 4.0]], np.float32), 2.0)[0, 0])
    assert S.stretched_lengths([12, 7, 5], 1.25, 10, 5).tolist() == [10, 6, 5]


BAD_RATES = [float('nan'), 0, 0.2, 4.5, float('inf'), 'fast']


@pytest.mark.parametrize('rate', BAD_RATES)
def test_python_refuses_a_bad_rate_before_any_device_call(rate):
    H = pkg('_hip')
    I = pkg('tacotron.inference')   # noqa: E741
    V = pkg('tacotron.serve')
    eng = no_device_engine()
    mag = np.ones((2, 3, 4), np.float32)
    ids = np.ones((2, 5), np.int32)
    with pytest.raises(ValueError):
        H.speaking_rate_value(rate)
    with pytest.raises(ValueError):
        eng.stretch_magnitudes(mag, rate)
    with pytest.raises(ValueError):
        eng.stretch_rows(mag, rate)
    with pytest.raises(ValueError):
        eng.stretched_frames(4, rate)
    with pytest.raises(ValueError):
        eng.set_speaking_rate(rate)
    with pytest.raises(ValueError):
        eng.time_stretch(np.zeros(4096, np.float32), rate)
    with pytest.raises(ValueError):
        eng.synthesize(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, speaking_rate=rate)
    with pytest.raises(ValueError):
        eng.synthesize_host(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, speaking_rate=rate)
    # the helpers validate before anything is loaded: no model, no weights, no engine exists here
    with pytest.raises(ValueError):
        I.synthesize_batch(None, ids, speaking_rate=rate)
    with pytest.raises(ValueError):
        next(I.synthesize_stream(None, [ids], speaking_rate=rate))
    with pytest.raises(ValueError):
        I.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', speaking_rate=rate)
    with pytest.raises(ValueError):
        next(V.serve(iter([['x']]), '/nonexistent/weights', speaking_rate=rate))
    with pytest.raises(ValueError):
        V.post_process_spectrograms(np.zeros((1, 40, 1025), np.float32), None, speaking_rate=rate)


def test_python_refuses_wrong_frame_counts_before_any_device_call():
    H = pkg('_hip')
    eng = no_device_engine()
    mag = np.ones((3, 5, 12), np.float32)
    for bad in [[12, 7], [[12, 7, 1]], [12, 7, 1, 1], 12, [12, 0, 1], [12, 13, 1], [12.0, 7.0, 1.0]]:
        with pytest.raises(ValueError):
            H.stretch_frame_counts(bad, 3, 12)
        with pytest.raises(ValueError):
            eng.stretch_magnitudes(mag, 1.3, n_frames=bad)
        with pytest.raises(ValueError):
            eng.stretch_rows(mag.transpose(0, 2, 1), 1.3, n_frames=bad)
    with pytest.raises(ValueError):
        eng.stretch_magnitudes(mag, 1.3, n_frames=[12, 7, 1], T_out=9)      # ceil(12 / 1.3) = 10
    with pytest.raises(ValueError):
        eng.stretch_magnitudes(np.ones((5, 12), np.float32), 1.3)
    assert H.stretch_frame_counts(None, 3, 12) is None
    got = H.stretch_frame_counts(np.array([12, 7, 1], np.int64), 3, 12)
    assert got.dtype == np.int32 and got.tolist() == [12, 7, 1]
    assert H.speaking_rate_value(None) is None and H.speaking_rate_value(1) == 1.0 and H.speaking_rate_value(np.float32(0.25)) == 0.25


def test_command_line_parses_and_checks_the_rate(tmp_path):
    I = pkg('tacotron.inference')   # noqa: E741
    assert I.parse_args([]).rate == 1.0
    assert I.parse_args(['--rate', '1.2']).rate == 1.2
    with pytest.raises(SystemExit):
        I.parse_args(['--rate', 'quick'])
    # main() checks the rate before it looks at a folder, a sentence file or a checkpoint
    for bad in ['nan', '0', '0.2', '4.5']:
        with pytest.raises(ValueError, match='speaking_rate'):
            I.main(['--rate', bad, '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])
    with pytest.raises(NotADirectoryError):   # a legal rate gets as far as the reference's first check
        I.main(['--rate', '1.2', '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])


def test_the_effects_module_points_to_the_engine():
    E = pkg('audio.effects')
    assert 'Engine.time_stretch' in E.__doc__ and 'pitch_shift' in E.__doc__
