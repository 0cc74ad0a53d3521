"""Loudness after ITU-R BS.1770-4 without a GPU: the K-weighting coefficients the library designs (tts_loudness_filter) against the
formulas and the standard's 48 kHz tables; the segmented oracle of tests/loudness_oracle.py -- the arithmetic the kernels are held
to bit for bit -- against its plain restatement (scipy's sosfilt over the whole signal); the standard's calibration tone and the
two gates; the symbols, the refusals of the library and of the Python surface made before a device is touched; the command
lines."""
import ctypes

import numpy as np
import pytest

import loudness_cases as C
import loudness_oracle as O
from conftest import pkg
from host_checks import no_device_engine


def _coeffs(sr):
    return pkg('_hip').loudness_filter(sr)


# ---------------------------------------------------------------------------------------------- the coefficients
@pytest.mark.parametrize('sr', [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 192000])
def test_the_coefficients_follow_the_formulas(sr):
    got, want = _coeffs(sr), O.design(sr)
    # tan and pow may differ in their last bit between libms, and the quotients pass that on: 4 ulp
    assert np.all(np.abs(got - want) <= 4 * np.spacing(np.abs(want))), (sr, got - want)
    assert tuple(got[5:8]) == (1.0, -2.0, 1.0)              # the high-pass numerator is not normalised, as in the standard


def test_the_coefficients_at_48_khz_are_the_standards_tables():
    assert np.abs(_coeffs(48000) - np.array(O.TABLE_48K)).max() <= 1e-14
    assert np.abs(O.design(48000) - np.array(O.TABLE_48K)).max() <= 1e-14


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.fixture(scope='module')
def measured():
    """every case once: name -> (sr, x, (z, J, passed) of the segmented oracle, z of the restatement)"""
    out = {}
    for name, sr, x in C.all_cases():
        k = _coeffs(sr)
        out[name] = (sr, x, O.mean_square(x, sr, k), O.plain_mean_square(x, sr, k))
    return out


def test_the_segmented_oracle_is_the_plain_restatement(measured):
    assert len(measured) == len(C.MEASURE) + len(C.TONE_RATES) + 2
    for name, (sr, x, (z, J, passed), plain) in measured.items():
        assert J == O.blocks(len(x), sr) and 0 <= passed <= J, name
        if J == 0:
            assert z == 0.0 and plain == 0.0, name
        else:
            # accumulated double rounding over 1e5 samples is of order 1e-11: 1e-9 is a hundred times that, and 4e-9 dB
            assert z > 0 and abs(z - plain) <= 1e-9 * plain, (name, z, plain)


def test_the_calibration_tone(measured):
    """a full-scale 997 Hz sine reads -3.01 LUFS at 48 kHz, the standard's calibration; the warped designs cost a few hundredths"""
    want = {48000: -3.0103, 44100: -3.0075, 22050: -2.9809, 16000: -2.9700, 8000: -2.9961}
    for sr in C.TONE_RATES:
        _sr, x, (z, _J, _p), _plain = measured['sine_%d' % sr]
        got = float(O.lufs(z))
        assert abs(got - (-3.0103)) <= (0.001 if sr == 48000 else 0.05), (sr, got)
        assert abs(got - want[sr]) <= 1e-4, (sr, got)          # the figures computed when the stage was specified
        half = O.mean_square(C.sine(sr, amplitude=0.5), sr, _coeffs(sr))[0]
        assert abs((got - float(O.lufs(half))) - 20.0 * np.log10(2.0)) <= 1e-9, sr


def test_the_gates(measured):
    k = _coeffs(16000)
    for name, rounded in (('relative_gate', -23.35), ('absolute_gate', -23.57)):
        _sr, x, (z, J, passed), plain = measured[name]
        assert 0 < passed < J, name
        assert abs(float(O.lufs(z)) - float(O.lufs(plain))) <= 1e-6
        assert round(float(O.lufs(z)), 2) == rounded
        ungated = float(O.lufs(O.plain_mean_square(x, 16000, k, gated=False)))
        assert ungated < float(O.lufs(z)) - 1.0, (name, ungated)          # the gate works: the quiet blocks pulled it down
    # the relative gate alone drops the -36 LUFS blocks of the first signal: every block passes the absolute one
    zb = O.plain_block_means(C.relative_gate_signal(), 16000, k)
    assert np.all(zb > O.Z_ABS)
    # the absolute gate alone drops the silent blocks of the second
    zb = O.plain_block_means(C.absolute_gate_signal(), 16000, k)
    assert 0 < np.sum(zb <= O.Z_ABS) < len(zb)


def test_the_special_cases_of_the_oracle():
    k = _coeffs(C.SR)
    s = O.step(C.SR)
    x = C.speech_like(6 * s + 100, C.SR)
    z = O.mean_square(x, C.SR, k)
    bad = x.copy()
    bad[3 * s] = np.nan
    assert np.isnan(O.mean_square(bad, C.SR, k)[0]) and O.mean_square(bad, C.SR, k)[1:] == (3, 0)
    behind = x.copy()
    behind[6 * s + 5] = np.inf
    assert O.mean_square(behind, C.SR, k) == z
    assert O.mean_square(np.zeros(6 * s, np.float32), C.SR, k) == (0.0, 3, 0)
    assert O.gain(0.0, 1.0, -23.0, 1.0) == 1.0 and O.gain(float('nan'), 1.0, -23.0, 1.0) == 1.0 and O.gain(0.1, 0.0, -23.0, 1.0) == 1.0
    assert O.gain(0.25, 0.5, -23.0, 1.0) == np.sqrt(10.0 ** ((-23.0 + 0.691) / 10.0) / 0.25)
    assert O.gain(1e-6, 0.5, -3.0, 0.25) == 0.5
    assert O.lufs(0.0) == -np.inf and np.isnan(O.lufs(np.nan))


# ---------------------------------------------------------------------------------------------- the library, without a device
NAMES = ('tts_loudness', 'tts_loudness_normalize', 'tts_loudness_filter', 'tts_loudness_segment', 'tts_set_loudness')


def test_symbols():
    H = pkg('_hip')
    lib = H.load_library()
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, 'include', 'sstts_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in H.exported_symbols() and getattr(lib, name) is not None
        assert 'int {}('.format(name) in header
    for sr in (8000, 16000, 22050, 48000, 192000):
        assert lib.tts_loudness_segment(sr) == O.segment(sr)
    assert lib.tts_loudness_segment(22050) == 276 and lib.tts_loudness_segment(7999) == 0 and lib.tts_loudness_segment(192001) == 0
    out = (ctypes.c_double * 10)()
    assert lib.tts_loudness_filter(7999, out) == H.TTS_ERR_UNSUPPORTED and lib.tts_loudness_filter(192001, out) == H.TTS_ERR_UNSUPPORTED
    assert lib.tts_loudness_filter(48000, None) == H.TTS_ERR_INVALID
    assert (H.LOUDNESS_SR_MIN, H.LOUDNESS_SR_MAX) == (O.SR_MIN, O.SR_MAX)


def _i32(values):
    arr = (ctypes.c_int32 * len(values))(*values)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), arr


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal is made on the arguments alone, ahead of the handle: with a NULL handle a bad call and a good one are both
    refused, but only the bad one with its own code and reason.  The pointers are never dereferenced."""
    H = pkg('_hip')
    lib = H.load_library()
    INV, UNS = H.TTS_ERR_INVALID, H.TTS_ERR_UNSUPPORTED
    p = 4096   # any aligned non-NULL address
    nan, inf = float('nan'), float('inf')

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    good, _k = _i32([5000, 1, 275])
    assert lib.tts_loudness(None, p, 3, 5000, good, 22050, p, p) == INV              # a good call: only the handle is missing
    for args, code, text in (
            ((None, 3, 5000, None, 22050, p, None), INV, 'loudness: a NULL pointer'),
            ((p, 3, 5000, None, 22050, None, None), INV, 'loudness: a NULL pointer'),
            ((p, 0, 5000, None, 22050, p, None), INV, 'loudness: need B, N >= 1'),
            ((p, 3, 0, None, 22050, p, None), INV, 'loudness: need B, N >= 1'),
            ((p, 3, 5000, _i32([5000, 0, 275])[0], 22050, p, None), INV, 'loudness: n_samples[1] = 0 is not in 1 .. N = 5000'),
            ((p, 3, 5000, _i32([5000, 1, 5001])[0], 22050, p, None), INV, 'loudness: n_samples[2] = 5001 is not in 1 .. N = 5000'),
            ((p, 3, 5000, None, 7999, p, None), UNS, 'loudness: the sampling rate 7999 is not in 8000 .. 192000'),
            ((p, 3, 5000, None, 192001, p, None), UNS, 'loudness: the sampling rate 192001 is not in 8000 .. 192000'),
            ((p + 2, 3, 5000, None, 22050, p, None), INV, 'loudness: mean_square must be 8-byte aligned'),
            ((p, 3, 5000, None, 22050, p + 4, None), INV, 'loudness: mean_square must be 8-byte aligned')):
        assert lib.tts_loudness(None, *args) == code and why().startswith(text), (args, why())
    assert lib.tts_loudness_normalize(None, p, 3, 5000, good, 22050, -23.0, 1.0, None, None) == INV
    for args, code, text in (
            ((None, 3, 5000, None, 22050, -23.0, 1.0, None, None), INV, 'loudness_normalize: a NULL pointer (wav is required)'),
            ((p, 3, 5000, None, 22050, nan, 1.0, None, None), INV, 'loudness_normalize: the target must be a finite number of LUFS'),
            ((p, 3, 5000, None, 22050, -inf, 1.0, None, None), INV, 'loudness_normalize: the target must be a finite number of LUFS'),
            ((p, 3, 5000, None, 22050, -23.0, 0.0, None, None), INV, 'loudness_normalize: max_peak must be finite and positive'),
            ((p, 3, 5000, None, 22050, -23.0, inf, None, None), INV, 'loudness_normalize: max_peak must be finite and positive'),
            ((p, 3, 5000, None, 22050, -23.0, nan, None, None), INV, 'loudness_normalize: max_peak must be finite and positive'),
            ((p, 3, 5000, _i32([5000, -1, 275])[0], 22050, -23.0, 1.0, None, None), INV, 'loudness_normalize: n_samples[1] = -1 is not in'),
            ((p, 3, 5000, None, 200000, -23.0, 1.0, None, None), UNS, 'loudness_normalize: the sampling rate 200000 is not in'),
            ((p, 3, 5000, None, 22050, -23.0, 1.0, p + 4, None), INV, 'loudness_normalize: mean_square and gain must be 8-byte aligned'),
            ((p, 3, 5000, None, 22050, -23.0, 1.0, None, p + 4), INV, 'loudness_normalize: mean_square and gain must be 8-byte aligned')):
        assert lib.tts_loudness_normalize(None, *args) == code and why().startswith(text), (args, why())
    assert lib.tts_set_loudness(None, 1, -23.0, 1.0, 22050) == INV


# ---------------------------------------------------------------------------------------------- the Python surface
def test_the_python_surface_refuses_before_it_touches_a_handle():
    H = pkg('_hip')
    eng = no_device_engine()
    X = np.zeros((2, 5000), np.float32)
    for call, text in (
            (lambda: eng.loudness(X, 7999), 'loudness: the sampling rate must be an integer in 8000 .. 192000, got 7999'),
            (lambda: eng.loudness(X, 22050.5), 'loudness: the sampling rate must be an integer in 8000 .. 192000, got 22050.5'),
            (lambda: eng.loudness(X, None), 'loudness: the sampling rate must be an integer in 8000 .. 192000, got None'),
            (lambda: eng.loudness(np.zeros((1, 2, 3), np.float32), 22050), 'loudness: one waveform (n,) or a batch (B, n) is needed, got shape (1, 2, 3)'),
            (lambda: eng.loudness(X, 22050, n_samples=[5000, 0]), 'n_samples[1] = 0 is not in 1 .. n = 5000'),
            (lambda: eng.loudness(X, 22050, n_samples=[5000, 5001]), 'n_samples[1] = 5001 is not in 1 .. n = 5000'),
            (lambda: eng.loudness(X, 22050, n_samples=[5000]), 'n_samples: 2 integers are needed, got shape (1,) of int64'),
            (lambda: eng.loudness_normalize(X, 192001), 'loudness_normalize: the sampling rate must be an integer in 8000 .. 192000, got 192001'),
            (lambda: eng.loudness_normalize(X, 22050, float('nan')), 'loudness_normalize: the target must be a finite number of LUFS, got nan'),
            (lambda: eng.loudness_normalize(X, 22050, -23.0, 0.0), 'loudness_normalize: max_peak must be finite and positive, got 0.0'),
            (lambda: eng.loudness_normalize(X, 22050, -23.0, float('inf')), 'loudness_normalize: max_peak must be finite and positive, got inf'),
            (lambda: eng.loudness_normalize(X, 22050, 'loud'), "loudness_normalize: target_lufs and max_peak must be numbers, got 'loud', 1.0"),
            (lambda: eng.set_loudness(float('inf')), 'loudness: the target must be a finite number of LUFS, got inf'),
            (lambda: eng.set_loudness((-23.0, -1.0)), 'loudness: max_peak must be finite and positive, got -1.0'),
            (lambda: eng.set_loudness((-23.0, 1.0, 2.0)), 'loudness must be None, a target in LUFS or (target_lufs, max_peak), got (-23.0, 1.0, 2.0)'),
            (lambda: eng.set_loudness(-23.0, sampling_rate=100), 'set_loudness: the sampling rate must be an integer in 8000 .. 192000, got 100')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert H.loudness_setting(None) is None and H.loudness_setting(-16) == (-16.0, 1.0) and H.loudness_setting((-23, 0.5)) == (-23.0, 0.5)
    assert H.lufs(0.0) == -np.inf and np.isnan(H.lufs(np.nan)) and abs(H.lufs(1.0) + 0.691) < 1e-15
    # the synthesis calls check the keyword before anything else is looked at
    ids = np.zeros((1, 4), np.int32)
    for bad in (float('nan'), (-23.0, 0.0), 'loud', (1, 2, 3)):
        with pytest.raises(ValueError):
            eng.synthesize(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, loudness=bad)
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.0, 100.0, 1.3, 3, 1102, 275, loudness=bad)


def test_the_keyword_is_threaded_through_the_entry_points():
    import inspect
    inf, serve = pkg('tacotron.inference'), pkg('tacotron.serve')
    H = pkg('_hip')
    for fn in (H.Engine.synthesize, H.Engine.synthesize_host, inf.synthesize_batch, inf.synthesize_stream, inf.synthesize_sentences,
               serve.serve, serve.post_process_spectrograms):
        assert inspect.signature(fn).parameters['loudness'].default is None, fn
    # ... and refused before a model is made
    for bad in (float('nan'), (-23.0, 0.0)):
        with pytest.raises(ValueError):
            inf.synthesize_batch(None, None, loudness=bad)
        with pytest.raises(ValueError):
            next(inf.synthesize_stream(None, [], loudness=bad))
        with pytest.raises(ValueError):
            inf.synthesize_sentences(['a'], None, loudness=bad)
        with pytest.raises(ValueError):
            next(serve.serve(iter([]), None, loudness=bad))
    assert 'tts_loudness' in pkg('audio.metrics').integrated_loudness.__doc__ or 'Engine.loudness' in pkg('audio.metrics').integrated_loudness.__doc__
    assert inspect.signature(pkg('audio.effects').normalize_loudness).parameters['target_lufs'].default == -23.0
    assert inspect.signature(pkg('datasets.statistics').collect_loudness).parameters['batch_size'].default == 32


def test_the_command_line_parses():
    inf = pkg('tacotron.inference')
    args = inf.parse_args([])
    assert args.loudness is None and args.max_peak == 1.0
    args = inf.parse_args(['--loudness', '-16', '--max-peak', '0.9'])
    assert (args.loudness, args.max_peak) == (-16.0, 0.9)
    assert inf.parse_args(['--loudness=-23']).loudness == -23.0
    with pytest.raises(SystemExit):
        inf.parse_args(['--loudness'])


# ---------------------------------------------------------------------------------------------- the wrappers, on the oracle
class _OracleEngine(object):
    """Engine.loudness / loudness_normalize answered by the oracle"""

    def loudness(self, wavs, sampling_rate, n_samples=None, return_mean_square=False, want_blocks=False):
        wavs = np.asarray(wavs, np.float32)
        rows = wavs[None] if wavs.ndim == 1 else wavs
        lens = [rows.shape[1]] * len(rows) if n_samples is None else list(n_samples)
        z = np.array([O.mean_square(r[:n], sampling_rate, _coeffs(sampling_rate))[0] for r, n in zip(rows, lens)])
        return O.lufs(z)


def _write_wav(path, x, sr):
    pkg('audio.io').save_wav(str(path), x, sr)


def test_integrated_loudness_and_collect_loudness(tmp_path):
    M, St = pkg('audio.metrics'), pkg('datasets.statistics')
    eng = _OracleEngine()
    x = C.tone_at(-20.0, 1.0, 16000)
    one = M.integrated_loudness(x, 16000, engine=eng)
    assert isinstance(one, float) and abs(one - (-20.0)) < 0.05
    both = M.integrated_loudness(np.stack([x, 0.5 * x]), 16000, engine=eng)
    assert both.shape == (2,) and abs((both[0] - both[1]) - 20.0 * np.log10(2.0)) < 1e-6
    paths = []
    for i, (level, seconds, sr) in enumerate([(-20.0, 1.0, 16000), (-30.0, 0.7, 16000), (-26.0, 0.5, 8000), (-20.0, 0.2, 16000)]):
        paths.append(str(tmp_path / ('%d.wav' % i)))
        _write_wav(paths[-1], C.tone_at(level, seconds, sr), sr)
    out = St.collect_loudness(paths, batch_size=3, engine=eng)
    assert out['lufs'].shape == (4,) and out['measured'] == 3 and out['lufs'][3] == -np.inf       # 0.2 s: no block
    assert np.all(np.abs(out['lufs'][:3] - np.array([-20.0, -30.0, -26.0])) < 0.05)
    fin = out['lufs'][:3]
    assert (out['min'], out['max']) == (fin.min(), fin.max()) and abs(out['mean'] - fin.mean()) < 1e-12 and abs(out['std'] - fin.std()) < 1e-12
    empty = St.collect_loudness(paths[3:], engine=eng)
    assert empty['measured'] == 0 and np.isnan(empty['mean'])


def test_dataset_statistics_prints_what_it_printed_and_the_loudness_behind_it(monkeypatch, capsys, tmp_path):
    D = pkg('tacotron.dataset_statistics')

    class _Dataset(object):
        _char2idx_dict = {'pad': 0, 'eos': 1, 'a': 2}

        def __init__(self, **kw):
            pass

        def load(self):
            return None, None, ['one.wav', 'two.wav']

    monkeypatch.setattr(D, 'LJSpeechDatasetHelper', _Dataset)
    monkeypatch.setattr(D, 'collect_decibel_statistics', lambda paths: (-100.0, 35.5, -99.25, 6.0))
    monkeypatch.setattr(D, 'collect_loudness', lambda paths: dict(lufs=np.array([-20.0, -24.0]), measured=2, min=-24.0, max=-20.0,
                                                                   mean=-22.0, std=2.0))
    before = ("Dataset: {0}\nLoading dataset ...\nDataset vocabulary:\nvocabulary_dict={{\n    'pad': 0,\n    'eos': 1,\n    'a': 2,\n}},\n"
              "vocabulary_size=3\n\n\n\nCollecting decibel statistics for 2 files ...\nmel_mag_ref_db =  6.0\nmel_mag_max_db =  -99.25\n"
              "linear_ref_db =  35.5\nlinear_mag_max_db =  -100.0\n").format(str(tmp_path))
    assert D.main(['--dataset-folder', str(tmp_path)]) == 0
    assert capsys.readouterr().out == before
    assert D.main(['--dataset-folder', str(tmp_path), '--loudness']) == 0
    out = capsys.readouterr().out
    assert out.startswith(before)
    assert out[len(before):] == ('Collecting loudness statistics for 2 files ...\nloudness_lufs_min =  -24.0\nloudness_lufs_max =  -20.0\n'
                                 'loudness_lufs_mean =  -22.0\nloudness_lufs_std =  2.0\nloudness_measured = 2 of 2\n')
