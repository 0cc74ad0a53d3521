"""Host: the resampler's oracle (tests/resample_oracle.py, resampy 0.2 resample_f with the 'kaiser_best' filter regenerated from its
published design) against its own properties, the bound of the GPU tests against its model, and the surface of the feature that
needs no device: lengths, refusals, option parsing.  librosa and resampy are not installed: the oracle is the yardstick, and
scipy's polyphase resampler with an independent Kaiser design is a gross-error guard only."""
import ctypes

import numpy as np
import pytest

import resample_cases as K
import resample_oracle as R
from conftest import pkg
from host_checks import no_device_engine

EDGE = 400      # samples at each end of a result that the filter's run-in reaches (64 zero crossings: 256 outputs at ratio 4)
N_IN = 8000


def _inner(y):
    assert y.shape[0] > 2 * EDGE + 100
    return y[EDGE:-EDGE]


@pytest.mark.parametrize('rho', K.CLEAN_RATIOS)
def test_dc_and_a_sine_come_back(rho):
    y, _ = R.resample(np.ones(N_IN), rho)
    dc = float(np.abs(_inner(y) - 1.0).max())
    t = np.arange(N_IN)
    y, _ = R.resample(np.sin(2 * np.pi * 0.05 * t), rho)
    want = np.sin(2 * np.pi * 0.05 * np.arange(y.shape[0]) * float(R.consts(rho)[2]))
    sine = float(np.abs(_inner(y) - _inner(want)).max())
    print('rho {:.4f}: DC error {:.2e}, sine error {:.2e}'.format(rho, dc, sine))
    assert dc <= 1e-6 and sine <= 1e-6


@pytest.mark.parametrize('rho', K.TRUNCATED_RATIOS)
def test_the_truncated_step_is_kept(rho):
    """step = int(scale * 512) is resampy's: the taps then sit a little closer than the filter's zero crossings, and DC comes
    back 3.4e-4 (2 ** (-4 / 12)) and 5.7e-4 (16000 / 22050) off"""
    scale, step, _inc = R.consts(rho)
    assert step < scale * R.NUM_TABLE
    y, _ = R.resample(np.ones(N_IN), rho)
    dc = float(np.abs(_inner(y) - 1.0).max())
    print('rho {:.4f}: DC error {:.2e}'.format(rho, dc))
    assert 1e-4 <= dc <= 1e-3


def test_an_independent_design_agrees():
    from scipy import signal
    rng = np.random.default_rng(3)
    b = signal.firwin(201, 0.4)
    x = np.convolve(rng.standard_normal(6000), b, mode='same')
    y, _ = R.resample(x, 2.0)
    want = signal.resample_poly(x, 2, 1, window=('kaiser', 14.0))
    err = float(np.linalg.norm(_inner(y) - _inner(want)) / np.linalg.norm(_inner(want)))
    print('rel-L2 against resample_poly: {:.2e}'.format(err))
    assert err < 1e-3


def test_lengths_and_layout():
    for n in (1, 2, 63, 441, 5000, 22050):
        for rho in K.RATIOS:
            y, s = R.resample(np.ones(n), rho)
            assert y.shape == s.shape == (R.resampled_length(n, rho),)
            keep = R.resampled_valid(n, rho)
            assert keep <= y.shape[0] <= keep + 1 and not y[keep:].any()
    assert R.resampled_valid(441, 16000.0 / 22050.0) == 320 and R.resampled_length(441, 16000.0 / 22050.0) == 320
    assert R.resampled_valid(3, 0.25) == 0 and R.resampled_length(3, 0.25) == 1
    y, s = R.resample_batch(np.ones((2, 10)), 2.0, [10, 3], n_out=25)
    assert y.shape == (2, 25) and not y[0, 20:].any() and not y[1, 6:].any() and y[1, 5] != 0


# ---------------------------------------------------------------------------------------------- the bound's model
def _cases(rho):
    x = np.nan_to_num(K.ragged_batch().astype(np.float64), nan=0.0)
    for b, n in enumerate(K.RAGGED):
        yield 'ragged[{}]'.format(b), x[b, :n]
    imp = K.impulse_batch().astype(np.float64)
    for b in range(imp.shape[0]):
        yield 'impulse[{}]'.format(b), imp[b]


@pytest.mark.parametrize('rho', K.RATIOS, ids=K.RATIO_IDS)
def test_what_the_bound_allows_stays_a_hundredfold_inside(rho):
    """another order of summation and a table that is 1e-14 (relative) off -- what a device's double arithmetic and its libm may
    differ by -- use less than a hundredth of the bound's accumulation term on every case"""
    worst = 0.0
    for name, x in _cases(rho):
        y, sabs = R.resample(x, rho)
        lim = 2.0 ** -36 * sabs / 100.0
        for variant in (dict(reverse=True), dict(table_eps=1e-14)):
            z, _ = R.resample(x, rho, **variant)
            err = np.abs(z - y)
            assert (err <= lim).all(), (name, variant)
            worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
    print('rho {:.4f}: worst error / (bound / 100) = {:.3f}'.format(rho, worst))


@pytest.mark.parametrize('rho', K.RATIOS, ids=K.RATIO_IDS)
def test_what_the_bound_must_catch_falls_outside(rho):
    """one tap dropped, eta forced to 0, m off by one: each leaves the bound on the impulse cases.  At 0.25, 0.5, 1, 2 and 4
    every output sits on a table sample (t / rho times 512 scale is an integer), so eta IS 0 there and forcing it changes
    nothing: that is asserted instead, and the forced eta is held to fall outside at the three ratios that interpolate."""
    imp = K.impulse_batch().astype(np.float64)
    taps_max = R.NWIN // R.consts(rho)[1]
    _m, (_o0, eta_l, _k0), (_o1, eta_r, _k1) = R.phase(np.arange(R.resampled_valid(K.IMPULSE_N, rho)), K.IMPULSE_N, rho)
    on_the_grid = rho in (0.25, 0.5, 1.0, 2.0, 4.0)
    assert on_the_grid == (not eta_l.any() and not eta_r.any())
    mistakes = [dict(m_shift=1), dict(m_shift=-1)] + ([] if on_the_grid else [dict(eta_zero=True)])
    # the taps an impulse can show: output t reads sample `at` through left tap m - at or right tap at - m - 1 (at ratio 0.25,
    # m = 4 t, the five impulses never meet a left tap i = 1 mod 4).  The first two, the middle one and the last of each wing:
    m, (_o, _e, taps_l), (_o, _e, taps_r) = R.phase(np.arange(R.resampled_valid(K.IMPULSE_N, rho)), K.IMPULSE_N, rho)
    for wing in (0, 1):
        met = set()
        for at in K.IMPULSE_AT:
            i = m - at if wing == 0 else at - m - 1
            met.update(i[(i >= 0) & (i < (taps_l if wing == 0 else taps_r))].tolist())
        met = sorted(met)
        assert len(met) >= taps_max // 2 and met[0] == 0 and met[-1] >= taps_max - 2
        mistakes += [dict(drop_tap=(wing, i)) for i in (met[0], met[1], met[len(met) // 2], met[-1])]
    for kw in mistakes:
        caught = 0
        for b in range(imp.shape[0]):
            y, sabs = R.resample(imp[b], rho)
            z, _ = R.resample(imp[b], rho, **kw)
            caught += int((np.abs(z.astype(np.float32).astype(np.float64) - y) > R.bound(y, sabs)).sum())
        assert caught > 0, (rho, kw)


def test_the_bound_is_the_issues():
    y = np.array([1.0, -2.0, 0.0])
    s = np.array([4.0, 8.0, 0.0])
    assert np.array_equal(R.bound(y, s), 2.0 ** -24 * np.abs(y) + 2.0 ** -36 * s)


def test_covers_is_the_window():
    """the outputs a sample reaches are those whose result changes when the sample does"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300)
    for rho in (0.5, 2.0 ** (-4.0 / 12.0), 2.0):
        y, _ = R.resample(x, rho)
        z = x.copy()
        z[150] += 1.0
        y2, _ = R.resample(z, rho)
        keep = R.resampled_valid(300, rho)
        changed = (y2 != y)[:keep]
        cov = R.covers(300, rho, 150)
        assert not (changed & ~cov).any() and changed.sum() >= cov.sum() - 4      # (a weight may be exactly 0)


# ---------------------------------------------------------------------------------------------- the surface
def test_host_helpers_agree_with_the_oracle():
    H = pkg('_hip')
    for n in (1, 2, 63, 441, 5000, 22050, 275000):
        for rho in K.RATIOS:
            assert H.resampled_length(n, rho) == R.resampled_length(n, rho) and H.resampled_valid(n, rho) == R.resampled_valid(n, rho)
    assert H.pitch_frames(40, 1.0, 4.0 / 12.0) == 51 and H.pitch_frames(40, 1.0, -4.0 / 12.0) == 32
    assert H.pitch_frames(40, 1.2, 4.0 / 12.0) == int(np.ceil(40 / (1.2 * 2.0 ** (-4.0 / 12.0))))
    assert H.pitch_semitones_value(4) == 4.0 / 12.0 and H.pitch_semitones_value(-12) == -1.0 and H.pitch_octaves_value(None) is None


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), 0.0, 0.2, 4.5, -1.0, 'fast'])
def test_python_refuses_bad_ratios_before_any_device_call(bad):
    H = pkg('_hip')
    eng = no_device_engine()
    with pytest.raises(ValueError):
        H.resample_ratio_value(bad)
    with pytest.raises(ValueError):
        H.resampled_length(10, bad)
    with pytest.raises(ValueError):
        eng.resample(np.zeros((2, 10), np.float32), bad)
    with pytest.raises(ValueError):
        eng.resampled_length(10, bad)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), 1.5, -1.01, 'high'])
def test_python_refuses_bad_pitches_before_any_device_call(bad):
    H = pkg('_hip')
    I = pkg('tacotron.inference')   # noqa: E741
    V = pkg('tacotron.serve')
    eng = no_device_engine()
    ids = np.ones((2, 5), np.int32)
    with pytest.raises(ValueError):
        H.pitch_octaves_value(bad)
    with pytest.raises(ValueError):
        eng.set_pitch(bad)
    with pytest.raises(ValueError):
        eng.pitch_shift(np.zeros(4096, np.float32), 22050, bad)
    with pytest.raises(ValueError):
        eng.synthesize(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, pitch=bad)
    with pytest.raises(ValueError):
        eng.synthesize_host(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, pitch=bad)
    with pytest.raises(ValueError):
        I.synthesize_batch(None, ids, pitch=bad)
    with pytest.raises(ValueError):
        next(I.synthesize_stream(None, [ids], pitch=bad))
    with pytest.raises(ValueError):
        I.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', pitch=bad)
    with pytest.raises(ValueError):
        next(V.serve(iter([['x']]), '/nonexistent/weights', pitch=bad))
    with pytest.raises(ValueError):
        V.post_process_spectrograms(np.zeros((1, 40, 1025), np.float32), None, pitch=bad)


def test_python_refuses_wrong_shapes_and_lengths_before_any_device_call():
    eng = no_device_engine()
    x = np.zeros((3, 20), np.float32)
    for bad in [[20, 7], [[20, 7, 1]], 20, [20, 0, 1], [20, 21, 1], [20.0, 7.0, 1.0]]:
        with pytest.raises(ValueError):
            eng.resample(x, 2.0, n_samples=bad)
    with pytest.raises(ValueError):
        eng.resample(np.zeros((2, 3, 4), np.float32), 2.0)
    with pytest.raises(ValueError):
        eng.resample(x, 2.0, N_out=0)
    # a pitch whose 2 ** -octaves times the speaking rate leaves [0.25, 4] (2.5 * 2 = 5, 0.4 / 2 = 0.2): refused in Python where
    # it can be seen; 2.5 * 2 ** -1 = 1.25 is legal
    H = pkg('_hip')
    for rate, octaves in [(2.5, -1.0), (0.4, 1.0)]:
        with pytest.raises(ValueError):
            H.pitch_frames(40, rate, octaves)
        with pytest.raises(ValueError):
            pkg('tacotron.serve').post_process_spectrograms(np.zeros((1, 40, 1025), np.float32), None, speaking_rate=rate, pitch=octaves)
    assert H.pitch_frames(40, 2.5, 1.0) == 32


def test_the_c_entry_point_of_the_length_needs_no_device():
    H = pkg('_hip')
    lib = H.load_library()
    out = ctypes.c_int(-5)
    for n in (1, 441, 5000):
        for rho in K.RATIOS:
            assert lib.tts_resampled_length(n, rho, ctypes.byref(out)) == H.TTS_OK and out.value == R.resampled_length(n, rho)
    out = ctypes.c_int(-5)
    for n, rho in [(0, 1.0), (5, float('nan')), (5, float('inf')), (5, 0.2), (5, 4.5)]:
        assert lib.tts_resampled_length(n, rho, ctypes.byref(out)) == H.TTS_ERR_INVALID and out.value == -5
    assert lib.tts_set_pitch(None, 0.0) == H.TTS_ERR_INVALID
    assert lib.tts_resample(None, None, 1, 1, None, 1.0, 1, None) == H.TTS_ERR_INVALID


def test_command_line_parses_and_checks_the_pitch(tmp_path):
    I = pkg('tacotron.inference')   # noqa: E741
    assert I.parse_args([]).pitch == 0.0
    assert I.parse_args(['--pitch', '-4']).pitch == -4.0
    with pytest.raises(SystemExit):
        I.parse_args(['--pitch', 'high'])
    # main() checks the pitch before it looks at a folder, a sentence file or a checkpoint
    for bad in ['nan', '13', '-12.5', 'inf']:
        with pytest.raises(ValueError, match='pitch'):
            I.main(['--pitch', bad, '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])
    with pytest.raises(NotADirectoryError):   # a legal pitch gets as far as the reference's first check
        I.main(['--pitch', '4', '--synthesis-dir', str(tmp_path / 'missing'), '--synthesis-file', str(tmp_path / 'missing.txt')])


def test_the_module_level_effects_keep_raising_and_point_to_the_engine():
    E = pkg('audio.effects')
    io = pkg('audio.io')
    with pytest.raises(NotImplementedError):
        E.pitch_shift(np.zeros(10, np.float32), 22050, 0.5)
    with pytest.raises(NotImplementedError):
        E.time_stretch(np.zeros(10, np.float32), 1.2)
    assert 'Engine.pitch_shift' in E.__doc__ and 'Engine.time_stretch' in E.__doc__ and 'tts_resample' in E.__doc__
    x = np.zeros(10, np.float32)
    assert io.resample(x, 22050, 22050) is x      # librosa returns its input for equal rates
    with pytest.raises(ValueError):
        io.resample(x, 22050, 2000, engine=no_device_engine())
    with pytest.raises(ValueError):
        io.resample(np.zeros((2, 10), np.float32), 22050, 16000, engine=no_device_engine())
