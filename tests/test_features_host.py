"""Host side of the dataset feature pass: the float64 trim restatement on hand-computed cases, silence_interval_from_spectrogram,
the precalc entry point's arguments, refusals that need no GPU, and the C ABI of features.hip."""
import os
import re

import numpy as np
import pytest

import trim_oracle as T
from conftest import ROOT, pkg


def test_trim_all_zeros_keeps_everything():
    assert T.trim_bounds(np.zeros(3000, np.float32)) == (0, 3000)
    assert T.trim_bounds(np.zeros(5121, np.float32), top_db=40) == (0, 5121)


def test_trim_tone_between_silences():
    # frame k covers [512 k - 1024, 512 k + 1024): frames 2 .. 7 touch samples 2000 .. 2999
    y = np.zeros(5000, np.float32)
    y[2000:3000] = np.sin(0.1 * np.arange(1000))
    assert T.trim_bounds(y) == (2 * 512, 8 * 512)


def test_trim_end_is_clamped_to_the_length():
    y = np.zeros(5000, np.float32)
    y[3000:] = np.sin(0.1 * np.arange(2000))
    assert T.trim_bounds(y) == (4 * 512, 5000)   # frames 4 .. 9; (9 + 1) * 512 > 5000


def test_trim_threshold_depends_on_top_db():
    y = np.zeros(8192, np.float32)
    y[3000:5000] = np.sin(0.05 * np.arange(2000))
    y[500:700] = 1e-2 * np.sin(0.05 * np.arange(200))     # ~ -50 dB against the tone's frames (frames 0 .. 3)
    s60, _ = T.trim_bounds(y, 60)
    s40, _ = T.trim_bounds(y, 40)
    assert s60 == 0 and s40 == 4 * 512


def test_trim_of_a_recording_with_a_nan_is_empty():
    # frame k covers [512 k - 1024, 512 k + 1024): sample 2500 lies in frames 3 .. 6 only, yet the NaN reaches the maximum and
    # with it the reference level of every frame -- numpy finds no frame above the threshold
    y = np.zeros(5000, np.float32)
    y[2000:3000] = np.sin(0.1 * np.arange(1000))
    y[2500] = np.nan
    mse, db = T.frame_power_db(y)
    assert np.flatnonzero(np.isnan(mse)).tolist() == [3, 4, 5, 6] and np.isnan(db).all()
    assert T.trim_bounds(y) == (0, 0) and T.trim_bounds(y, top_db=20) == (0, 0)
    # ... wherever it is: in the first frame (through the reflection), in the last sample
    for pos in (0, 4999):
        y = np.zeros(5000, np.float32)
        y[2000:3000] = np.sin(0.1 * np.arange(1000))
        y[pos] = np.nan
        assert T.trim_bounds(y) == (0, 0)


def test_trim_of_a_recording_with_an_infinity_is_empty():
    # the frames that hold the sample are Inf - Inf = NaN against the reference level, the others finite - Inf = -Inf
    for value in (np.inf, -np.inf):
        y = np.zeros(5000, np.float32)
        y[2000:3000] = np.sin(0.1 * np.arange(1000))
        y[2500] = value
        mse, db = T.frame_power_db(y)
        assert np.flatnonzero(np.isinf(mse)).tolist() == [3, 4, 5, 6]
        assert np.isnan(db[3:7]).all() and np.isneginf(np.delete(db, [3, 4, 5, 6])).all()
        assert T.trim_bounds(y) == (0, 0)


def test_silence_interval_from_spectrogram():
    E = pkg('audio.effects')
    spec = np.full((5, 8), -80.0)
    spec[2, 3] = -10.0
    spec[4, 6] = -30.0
    assert E.silence_interval_from_spectrogram(spec, -40.0) == (3, 6)
    assert E.silence_interval_from_spectrogram(spec, -20.0) == (3, 3)
    assert E.silence_interval_from_spectrogram(spec, 0.0) is None


def test_effects_refusals():
    E = pkg('audio.effects')
    with pytest.raises(NotImplementedError):
        E.pitch_shift(np.zeros(10), 22050, 1)
    with pytest.raises(NotImplementedError):
        E.time_stretch(np.zeros(10), 1.1)
    with pytest.raises(NotImplementedError, match='np.max'):
        E.trim_silence(np.zeros(4000, np.float32), ref=np.mean)
    with pytest.raises(AssertionError, match='greater 0'):
        E.crop_silence_left(np.zeros(100), 1000, 0)
    with pytest.raises(AssertionError, match='total wav length'):
        E.crop_silence_right(np.zeros(100), 1000, 200)


def test_precalc_entry_point_arguments():
    M = pkg('tacotron.dataset_precalc_features')
    P = pkg('tacotron.params')
    a = M.parse_args([])
    assert a.dataset_folder == P.dataset_params.dataset_folder and a.batch_size == 32
    a = M.parse_args(['--dataset-folder', '/data/lj', '--batch-size', '48'])
    assert a.dataset_folder == '/data/lj' and a.batch_size == 48
    with pytest.raises(SystemExit):
        M.parse_args(['--batch-size', '0'])


def test_lj_helper_feature_constants_match_the_params_class():
    LJ = pkg('datasets.lj_speech').LJSpeechDatasetHelper
    C = pkg('tacotron.params').LJSpeechConstants
    for k in ('mel_mag_ref_db', 'mel_mag_max_db', 'linear_ref_db', 'linear_mag_max_db'):
        assert getattr(LJ, k) == getattr(C, k)


def test_feature_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'sstts_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    names = ('tts_trim_bounds', 'tts_default_feature_params', 'tts_plan_features', 'tts_extract_features')
    lib = pkg().load_library()
    for n in names:
        assert re.search(r'\b' + n + r'\s*\(', header), n
        assert n in pkg().exported_symbols()
        getattr(lib, n)


def test_default_feature_params_and_struct_size():
    H = pkg('_hip')
    lib = H.load_library()
    p = H.TtsFeatureParams()
    assert lib.tts_default_feature_params(p) == 0
    assert p.struct_size == __import__('ctypes').sizeof(H.TtsFeatureParams)
    assert (p.n_fft, p.win_length, p.hop_length, p.sampling_rate, p.n_mels, p.reduction) == (2048, 1102, 275, 22050, 80, 5)
    assert (p.trim, p.trim_top_db, p.trim_frame_length, p.trim_hop_length) == (1, 60.0, 2048, 512)
    assert abs(p.mel_ref_db - 6.02) < 1e-6 and abs(p.linear_ref_db - 35.66) < 1e-5 and p.fmax == 8000.0
