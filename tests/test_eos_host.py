"""Host side of end-of-speech stopping (no GPU): the oracle on hand-written cases, the threshold helper against its closed
forms, the refusals of the Python surface, the new symbols, and the end-to-end fixtures of test_gpu_eos.py held to their
off-threshold condition on the float64 network oracle (the device's float32 network differs from it by ~1e-5, the
condition asks for 1e-3)."""
import ctypes
import math
import os

import numpy as np
import pytest

import eos_cases as K
import eos_oracle as E
from conftest import ROOT, pkg

NEW_SYMBOLS = ['tts_speech_frames', 'tts_speech_threshold', 'tts_set_end_of_speech', 'tts_synth_frames', 'tts_wait_host_frames']


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_is_strict_at_equality():
    x = np.array([[0.1, 0.5, 0.2], [0.0, 0.3, 0.2]])   # (F, T): frame maxima 0.1, 0.5, 0.2
    assert E.silence_interval(x, 0.5) is None
    assert E.silence_interval(x, np.nextafter(0.5, 0)) == (1, 1)
    assert E.speech_frames(x, 0.5) == (1, -1)
    assert E.speech_frames(x, 0.2) == (2, 1)


def test_oracle_none_first_and_last_frame():
    x = np.zeros((4, 6))
    assert E.speech_frames(x, 0.0, keep_frames=2, min_frames=3) == (3, -1)
    x[2, 0] = 1.0
    assert E.silence_interval(x, 0.5) == (0, 0)
    assert E.speech_frames(x, 0.5) == (1, 0)
    assert E.speech_frames(x, 0.5, keep_frames=3) == (4, 0)
    assert E.speech_frames(x, 0.5, keep_frames=100) == (6, 0)
    x[1, 5] = 2.0
    assert E.silence_interval(x, 0.5) == (0, 5)
    assert E.speech_frames(x, 0.5, min_frames=6) == (6, 5)


def test_oracle_nan_column_is_silent_and_infinities_compare():
    x = np.zeros((3, 5))
    x[0, 1] = 1.0
    x[:, 3] = [np.nan, 9.0, 0.0]      # a NaN beside a value above the threshold: np.max is NaN, the comparison False
    x[:, 4] = -np.inf
    assert np.isnan(E.frame_maxima(x)[3])
    assert E.speech_frames(x, 0.5) == (2, 1)
    x[2, 2] = np.inf
    assert E.speech_frames(x, 0.5) == (3, 2)
    assert E.speech_frames(x, np.inf) == (1, -1)


def test_stage_fixture_holds_every_case_it_names():
    for F in K.STAGE_F:
        x = K.stage_batch(F)
        n, last = E.speech_frames_batch(x, K.STAGE_THRESHOLD)
        assert last.tolist() == K.STAGE_EXPECT_LAST and n.tolist() == [13, 1, 1, K.STAGE_T, 26]
        assert np.nanmax(x[0, 20]) == K.STAGE_THRESHOLD and np.isnan(x[0, 30]).any() and np.isneginf(x[0, 33]).all()
        if F > 1:
            assert np.nanmax(x[0, 30]) > K.STAGE_THRESHOLD and x[0, 3].argmax() == 0 and x[0, 12].argmax() == F - 1
        # the padding of the strided forms never counts: the oracle sees the first F columns only
        for fill in (np.nan, np.inf):
            full, view = K.padded(x, 3, fill)
            assert view.base is full and np.array_equal(E.speech_frames_batch(view, K.STAGE_THRESHOLD)[1], last)


# ---------------------------------------------------------------------------------------------- the threshold helper
@pytest.fixture(scope='module')
def lib():
    return pkg().load_library()


def _threshold(lib, db, ref, mx, power, units):
    out = ctypes.c_float()
    rc = lib.tts_speech_threshold(db, ref, mx, power, units, ctypes.byref(out))
    return rc, np.float32(out.value)


@pytest.mark.parametrize('db', [-40.0, -100.0, 0.0, 6.02, -53.153786, 12.5])
@pytest.mark.parametrize('ref,mx,power', [(6.02, 99.89, 1.3), (35.66, 100.0, 1.0), (-20.0, 80.0, 1.5)])
def test_threshold_helper_is_the_closed_form_in_double(lib, db, ref, mx, power):
    f = lambda v: float(np.float32(v))   # (the C entry point takes floats)  # noqa: E731
    rc, got = _threshold(lib, db, ref, mx, power, 0)
    assert rc == 0 and got == np.float32((f(db) - f(ref)) / (abs(f(ref)) + abs(f(mx))) + 1.0)
    rc, got = _threshold(lib, db, ref, mx, power, 1)
    assert rc == 0 and got == np.float32(math.pow(math.pow(10.0, f(db) / 20.0), f(power)))


def test_threshold_helper_inverts_the_denormalisation_and_is_monotone(lib):
    from oracle import audio_oracle as AO
    prev = (-np.inf, -np.inf)
    for db in np.linspace(-90.0, 6.0, 25):
        _, x = _threshold(lib, db, K.REF_DB, K.MAX_DB, K.POWER, 0)
        _, m = _threshold(lib, db, K.REF_DB, K.MAX_DB, K.POWER, 1)
        assert abs(AO.inv_normalize_decibel(np.float64(x), K.REF_DB, K.MAX_DB) - db) < 1e-4
        assert abs(m - np.power(AO.decibel_to_magnitude(np.float64(db)), K.POWER)) <= 1e-6 * m
        assert x > prev[0] and m > prev[1]
        prev = (x, m)


def test_threshold_helper_refusals(lib):
    nan = float('nan')
    assert _threshold(lib, nan, 6.02, 99.89, 1.3, 0)[0] == -1
    assert _threshold(lib, nan, 6.02, 99.89, 1.3, 1)[0] == -1
    assert _threshold(lib, -40.0, nan, 99.89, 1.3, 0)[0] == -1
    assert _threshold(lib, -40.0, 0.0, 0.0, 1.3, 0)[0] == -1
    assert _threshold(lib, -40.0, 6.02, 99.89, 0.0, 1)[0] == -1
    assert _threshold(lib, -40.0, 6.02, 99.89, nan, 1)[0] == -1
    assert _threshold(lib, -40.0, 6.02, 99.89, 1.3, 2)[0] == -1
    assert lib.tts_speech_threshold(-40.0, 6.02, 99.89, 1.3, 0, None) == -1
    # (what one units does not use may be anything)
    assert _threshold(lib, -40.0, nan, nan, 1.3, 1)[0] == 0 and _threshold(lib, -40.0, 6.02, 99.89, nan, 0)[0] == 0


# ---------------------------------------------------------------------------------------------- symbols, header
def test_new_entry_points_are_exported_and_documented(lib):
    H = pkg('_hip')
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in H.exported_symbols()
        assert getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    assert '"speech_end"' in header


def test_handle_free_refusals_of_the_c_entry_points(lib):
    n = (ctypes.c_int32 * 2)()
    assert lib.tts_speech_frames(None, None, 1, 1, 1, 1, 0.5, 0, 1, None, None) == -1
    assert lib.tts_set_end_of_speech(None, 1, -40.0, 0) == -1
    assert lib.tts_synth_frames(None, n, 2) == -1
    assert lib.tts_wait_host_frames(None, 0, None, None) == -1


# ---------------------------------------------------------------------------------------------- the Python surface
def test_stop_at_silence_setting_refusals():
    H = pkg('_hip')
    assert H.stop_at_silence_setting(None) is None
    assert H.stop_at_silence_setting((-40, 3)) == (-40.0, 3)
    assert H.stop_at_silence_setting([-40.5, np.int64(0)]) == (-40.5, 0)
    for bad in [(float('nan'), 0), (-40.0, -1), (-40.0, 1.5), -40.0, (-40.0,), (-40.0, 1, 2), ('x', 0)]:
        with pytest.raises(ValueError):
            H.stop_at_silence_setting(bad)


def test_silence_keep_ms_becomes_whole_frames():
    H = pkg('_hip')
    conv = pkg('audio.conversion')
    hop = conv.ms_to_samples(12.5, 22050)
    assert hop == 275
    for ms, frames in [(0.0, 0), (12.5, 1), (12.6, 2), (100.0, 9), (1000.0, 81)]:
        assert H.silence_keep_frames(conv.ms_to_samples(ms, 22050), hop) == frames
    for bad in (-1, float('nan')):
        with pytest.raises(ValueError):
            H.silence_keep_frames(bad, hop)
    I = pkg('tacotron.inference')   # noqa: E741
    P = pkg('tacotron.params')
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError):
            I.stop_setting(P.model_params, -40.0, bad)


def test_inference_helpers_and_command_line():
    I = pkg('tacotron.inference')   # noqa: E741
    P = pkg('tacotron.params')
    assert I.stop_setting(P.model_params, None, 100.0) is None
    assert I.stop_setting(P.model_params, -40, 100.0) == (-40.0, 9)
    with pytest.raises(ValueError):
        I.stop_setting(P.model_params, -40.0, -5.0)
    with pytest.raises(ValueError):
        I.stop_setting(P.model_params, float('nan'), 100.0)
    args = I.parse_args(['--stop-at-silence', '-40', '--silence-keep-ms', '50'])
    assert args.stop_at_silence == -40.0 and args.silence_keep_ms == 50.0
    args = I.parse_args([])
    assert args.stop_at_silence is None and args.silence_keep_ms == I.SILENCE_KEEP_MS
    wavs = np.arange(3 * 10, dtype=np.float32).reshape(3, 10)
    cut = I.cut_waveforms(wavs, [2, 6, 1], 2)
    assert [len(c) for c in cut] == [2, 10, 0] and np.array_equal(cut[0], wavs[0, :2])
    # refused before anything is loaded or a folder is looked at
    with pytest.raises(ValueError):
        I.synthesize_sentences(['a'], weights=None, out_dir='/nonexistent', stop_at_silence_db=-40.0, silence_keep_ms=-1.0)
    with pytest.raises(ValueError):
        next(pkg('tacotron.serve').serve(iter([['a']]), weights=None, stop_at_silence_db=-40.0, silence_keep_ms=-1.0))


# ---------------------------------------------------------------------------------------------- the GPU test's fixtures
@pytest.mark.parametrize('case', [K.E2E, K.E2E_512], ids=['2048', '512'])
def test_end_to_end_fixture_stays_off_the_threshold(case):
    """the ids and weights test_gpu_eos.py synthesises from, on the float64 network oracle: a threshold exists that gives
    three different lengths and lies at least 3 OFF_THRESHOLD from every frame's maximum -- so the device's float32
    network (~1e-5 from this one) finds a gap that satisfies the condition as well"""
    from oracle import tacotron_oracle as O
    hp = K.hparams_of(case)
    w = {k: v.astype(np.float64) for k, v in K.weights_of(case).items()}
    ref = O.tacotron_predict(K.ids_of(case), w, hp, n_steps=case['S'])
    lin = ref['linear'].astype(np.float32)
    thr = K.choose_threshold(lin, case['min_frames'])
    assert thr is not None
    n = K.oracle_lengths(lin, thr, 0, case['min_frames'])
    d = K.distance_from_threshold(lin, thr)
    print('n_fft {}: threshold {} dB, lengths {}, distance {:.2e}'.format(case['n_fft'], thr, n, d))
    assert len(set(n.tolist())) == case['B'] and n.min() >= case['min_frames'] and n.max() <= case['S'] * hp.reduction
    assert d >= 3 * K.OFF_THRESHOLD
    # and the extremes the GPU test also runs: below every value everything is active, above every value nothing is
    T = case['S'] * hp.reduction
    assert K.oracle_lengths(lin, -101.0, 0, case['min_frames']).tolist() == [T] * case['B']
    assert K.oracle_lengths(lin, K.REF_DB + 1.0, 0, case['min_frames']).tolist() == [case['min_frames']] * case['B']
