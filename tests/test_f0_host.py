"""F0 tracking without a GPU: the numpy oracle (tests/f0_oracle.py) against tones of known pitch, noise, silence and a NaN sample;
its vectorised decisions against the plain walks of the definition; the Python surface (audio.features.fundamental_frequency,
audio.metrics.f0_errors) on an engine whose two device calls are the oracles; the refusals of tts_f0 and tts_f0_compare -- which
return before a device is touched -- and the exported symbols."""
import ctypes

import numpy as np
import pytest

import f0_cases as K
import f0_oracle as Y
from conftest import pkg
from host_checks import no_device_engine

E = K.EVAL


def _interior(T, hop, n, W, tau_max):
    """frames whose span lies inside the signal"""
    half = (W + tau_max) // 2
    return [t for t in range(T) if t * hop - half >= 0 and t * hop - half + W + tau_max <= n]


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.fixture(scope='module')
def tone_tracks():
    n = 8800
    x = np.stack([K.tone(hz, n, seed=int(hz)) for hz in K.TONES_HZ])
    q, c_last = Y.normalised_difference(x, E['hop'], E['W'], E['tau_max'])
    return n, x, q, c_last


def test_tones_of_known_pitch(tone_tracks):
    n, x, q, c_last = tone_tracks
    f0, ap = Y.decide(q, c_last, K.SR, E['tau_min'], E['tau_max'], 0.1)
    inner = _interior(f0.shape[1], E['hop'], n, E['W'], E['tau_max'])
    assert len(inner) >= 20
    worst = 0.0
    for row, hz in enumerate(K.TONES_HZ):
        track = f0[row, inner].astype(np.float64)
        assert (track > 0).all(), hz
        worst = max(worst, np.abs(track / hz - 1.0).max())
    print('worst relative error over the interior frames: {:.2e}'.format(worst))
    assert worst <= 5e-4


def test_the_vectorised_decisions_are_the_walks(tone_tracks):
    n, x, q, c_last = tone_tracks
    rng = np.random.default_rng(5)
    noisy = (x + 0.3 * rng.standard_normal(x.shape)).astype(np.float32)
    noisy[1, 4000] = np.nan
    q2, c2 = Y.normalised_difference(noisy[:3], E['hop'], E['W'], E['tau_max'])
    for qq, cc in ((q, c_last), (q2, c2)):
        for thr in (0.1, 0.5, 0.0, float('inf')):
            f0, ap = Y.decide(qq, cc, K.SR, E['tau_min'], E['tau_max'], thr)
            for r in range(qq.shape[0]):
                for t in range(0, qq.shape[1], 3):
                    wf, wa = Y.decide_walk(qq[r, t], cc[r, t], K.SR, E['tau_min'], E['tau_max'], thr)
                    assert Y.same_bits(f0[r, t], wf) and Y.same_bits(ap[r, t], wa), (thr, r, t)


def test_white_noise_is_unvoiced():
    x = np.random.default_rng(1).standard_normal((1, 8800)).astype(np.float32)
    f0, ap = Y.f0(x, K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
    print('lowest aperiodicity of noise: {:.3f}'.format(ap.min()))
    assert (f0 == 0).all() and ap.min() > 0.5


def test_zeros_are_unvoiced_with_aperiodicity_one():
    f0, ap = Y.f0(np.zeros((1, 3000), np.float32), K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
    assert f0.shape == (1, 11) and (f0 == 0).all() and (ap == 1).all()


def test_a_nan_sample_spoils_exactly_the_frames_whose_span_holds_it():
    n, at = 8800, 4321
    x = K.tone(150.0, n)[None].copy()
    clean = Y.f0(x, K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
    x[0, at] = np.nan
    f0, ap = Y.f0(x, K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
    span = E['W'] + E['tau_max']
    for t in range(f0.shape[1]):
        s0 = Y.first_sample(t, E['hop'], E['W'], E['tau_max'])
        inside = s0 <= at < s0 + span
        assert np.isnan(f0[0, t]) == inside and np.isnan(ap[0, t]) == inside, t
        if not inside:
            assert Y.same_bits(f0[0, t], clean[0][0, t]) and Y.same_bits(ap[0, t], clean[1][0, t])
    assert np.isnan(f0).sum() == -(-span // E['hop']) or np.isnan(f0).sum() == span // E['hop']


def test_lengths_and_padding_frames():
    x = K.batch(700, 63)
    n_samples = [1, 7, 126, 699, 700, 350, 6, 8, 64, 65, 700]
    poisoned = x.copy()
    for b, n in enumerate(n_samples):
        poisoned[b, n:] = np.nan
    f0, ap = Y.f0(poisoned, K.SR, 7, 63, 2, 63, 0.1, n_samples=n_samples)
    for b, n in enumerate(n_samples):
        alone = Y.f0(x[b:b + 1, :n], K.SR, 7, 63, 2, 63, 0.1)
        Tb = Y.frames(n, 7)
        assert Y.same_bits(f0[b, :Tb], alone[0][0]) and Y.same_bits(ap[b, :Tb], alone[1][0])
        assert (f0[b, Tb:] == 0).all() and (ap[b, Tb:] == 0).all()


def test_the_comparison_oracle_counts_what_the_header_says():
    a, b = K.tracks(3, 40, 55)
    path = K.diagonal_path(40, 55, 94)
    counts, s_hz, s_cents, abs_z = Y.compare(a, b, path)
    assert counts[0] == 55 and counts[0] == counts[1] + counts[2] + counts[4] + 2    # two steps unvoiced on both sides
    assert counts[4] == 2 and counts[2] == 6
    assert counts[3] >= 2     # one float beyond the 20 % edge, and the two octaves; the pair at the edge itself is none
    only_edge = Y.compare(a[17:18], b[17:18], np.array([[0, 0]]))
    beyond = Y.compare(a[18:19], b[18:19], np.array([[0, 0]]))
    assert only_edge[0][3] == 0 and beyond[0][3] == 1
    assert s_hz > 0 and s_cents > 0 and abs_z > 0


# ---------------------------------------------------------------------------------------------- the Python surface
class _Host(object):
    """what Engine hands back: to_host() and free()"""

    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def to_host(self):
        return self.a

    def free(self):
        pass


class _OracleEngine(object):
    """an engine whose f0 and f0_compare are the numpy oracles: the layers above them run as they are"""

    def f0(self, wavs, sampling_rate, hop_length, fmin=60.0, fmax=500.0, window=1024, threshold=0.1, n_samples=None,
           want_aperiodicity=False):
        lo, hi = Y.lag_bounds(sampling_rate, fmin, fmax)
        f0, ap = Y.f0(wavs, sampling_rate, hop_length, window, lo, hi, threshold, n_samples)
        return (_Host(f0), _Host(ap)) if want_aperiodicity else _Host(f0)

    def f0_compare(self, f0_a, f0_b, path):
        B = f0_a.shape[0]
        counts, sums = np.zeros((B, 5), np.int32), np.zeros((B, 2))
        for p in range(B):
            counts[p], sums[p, 0], sums[p, 1], _ = Y.compare(f0_a[p], f0_b[p], path[p])
        return _Host(counts), _Host(sums)


def test_fundamental_frequency_returns_the_track_of_a_waveform():
    F = pkg('audio.features')
    x = K.tone(220.0, 5000)
    f0 = F.fundamental_frequency(x, K.SR, 275, engine=_OracleEngine())
    assert f0.shape == (19,) and f0.dtype == np.float32
    inner = _interior(19, 275, 5000, 1024, 368)
    assert len(inner) >= 8 and np.abs(f0[inner] / 220.0 - 1.0).max() <= 5e-4
    f0b, ap = F.fundamental_frequency(x, K.SR, 275, want_aperiodicity=True, engine=_OracleEngine())
    assert Y.same_bits(f0, f0b) and ap.shape == (19,) and ap[inner].max() < 0.1
    assert 'no reference counterpart' in F.fundamental_frequency.__doc__.lower()
    with pytest.raises(ValueError):
        F.fundamental_frequency(x[None], K.SR, 275, engine=_OracleEngine())


def test_f0_errors_are_the_textbook_figures():
    M = pkg('audio.metrics')
    a, b = K.tracks(3, 40, 55)
    path = K.diagonal_path(40, 55, 94)
    clean_a, clean_b = np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)
    out = M.f0_errors(np.stack([a, clean_a, np.zeros_like(a)]), np.stack([b, clean_b, clean_b]), np.stack([path] * 3),
                      engine=_OracleEngine())
    assert out['counts'].shape == (3, 5)
    # a NaN step: no RMSE; the other figures stand
    assert np.isnan(out['f0_rmse_hz'][0]) and np.isnan(out['f0_rmse_cents'][0]) and out['vuv_error'][0] > 0
    # the clean pair against a direct evaluation
    steps = [(i, j) for i, j in path.tolist() if i >= 0]
    fa = np.array([clean_a[i] for i, _ in steps], np.float64)
    fb = np.array([clean_b[j] for _, j in steps], np.float64)
    both = (fa > 0) & (fb > 0)
    assert out['counts'][1].tolist() == [len(steps), both.sum(), ((fa > 0) != (fb > 0)).sum(),
                                         (np.abs(fa - fb)[both] > 0.2 * fb[both]).sum(), 0]
    assert abs(out['f0_rmse_hz'][1] - np.sqrt(np.mean((fa - fb)[both] ** 2))) <= 1e-9
    assert abs(out['f0_rmse_cents'][1] - np.sqrt(np.mean((1200.0 * np.log2(fa[both] / fb[both])) ** 2))) <= 1e-9
    assert out['vuv_error'][1] == ((fa > 0) != (fb > 0)).sum() / len(steps)
    assert out['gross_pitch_error'][1] == (np.abs(fa - fb)[both] > 0.2 * fb[both]).sum() / both.sum()
    # nothing voiced on both sides: no RMSE, no gross pitch error, a voicing error
    assert np.isnan(out['f0_rmse_hz'][2]) and np.isnan(out['gross_pitch_error'][2]) and out['vuv_error'][2] > 0.5


# ---------------------------------------------------------------------------------------------- the library, without a device
def test_symbols():
    H = pkg('_hip')
    lib = H.load_library()
    for name in ('tts_f0', 'tts_f0_compare', 'tts_f0_frames', 'tts_f0_max_window', 'tts_f0_max_lag'):
        assert name in H.exported_symbols() and getattr(lib, name) is not None
    assert lib.tts_f0_max_window() == 2048 == H.F0_MAX_WINDOW and lib.tts_f0_max_lag() == 1024 == H.F0_MAX_LAG
    for n, hop in ((1, 1), (274, 275), (275, 275), (16500, 275), (5, 7)):
        assert lib.tts_f0_frames(n, hop) == 1 + n // hop == H.f0_frames(n, hop)
    assert H.f0_lag_bounds(22050, 60.0, 500.0) == (44, 368) == Y.lag_bounds(22050, 60.0, 500.0)


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

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    # tts_f0(h, wav, B, N, n_samples, sampling_rate, hop, W, tau_min, tau_max, threshold, f0, aperiodicity)
    good = [p, 3, 5000, None, 22050.0, 275, 1024, 44, 368, 0.1, p, None]
    for at, bad, word in [(0, None, 'NULL'), (10, None, 'NULL'), (1, 0, '>= 1'), (2, 0, '>= 1'), (5, 0, '>= 1'), (4, 0.0, 'sampling rate'),
                          (4, float('nan'), 'sampling rate'), (4, float('inf'), 'sampling rate'), (4, -8000.0, 'sampling rate'),
                          (9, float('nan'), 'threshold')]:
        args = list(good)
        args[at] = bad
        assert lib.tts_f0(None, *args) == INV and word in why() and why().startswith('f0: '), (at, bad, why())
    for lens in ([5000, 0, 1], [5001, 1, 1], [1, 1, -2]):
        ptr, keep = _i32(lens)
        args = list(good)
        args[3] = ptr
        assert lib.tts_f0(None, *args) == INV and 'n_samples[' in why(), lens
    for at, bad, word in [(6, 0, '2048'), (6, 2049, '2048'), (7, 1, '1024'), (8, 1025, '1024'), (7, 369, '1024')]:
        args = list(good)
        args[at] = bad
        assert lib.tts_f0(None, *args) == UNS and word in why() and why().startswith('f0: '), (at, bad, why())

    # tts_f0_compare(h, f0_a, Ta, f0_b, Tb, path, rows, B, counts, sums)
    good2 = [p, 40, p, 55, p, 94, 3, p, p]
    for at, bad, word in [(0, None, 'NULL'), (2, None, 'NULL'), (4, None, 'NULL'), (7, None, 'NULL'), (8, None, 'NULL'), (1, 0, '>= 1'),
                          (3, -1, '>= 1'), (5, 0, '>= 1'), (6, 0, '>= 1'), (8, p + 4, '8-byte')]:
        args = list(good2)
        args[at] = bad
        assert lib.tts_f0_compare(None, *args) == INV and word in why() and why().startswith('f0_compare: '), (at, bad, why())
    # legal calls: what is left is the missing handle, and no new reason
    before = why()
    ptr, keep = _i32([5000, 1, 275])
    args = list(good)
    args[3] = ptr
    assert lib.tts_f0(None, *args) == INV and why() == before
    args = list(good)
    args[6:9] = [2048, 2, 1024]
    args[9] = float('inf')
    assert lib.tts_f0(None, *args) == INV and why() == before
    assert lib.tts_f0_compare(None, *good2) == INV and why() == before


def test_python_refuses_bad_arguments_before_any_device_call():
    eng = no_device_engine()
    x = np.zeros((2, 5000), np.float32)
    with pytest.raises(ValueError, match='2048'):
        eng.f0(x, 22050, 275, window=2049)
    with pytest.raises(ValueError, match='1024'):
        eng.f0(x, 22050, 275, fmin=20.0)        # ceil(22050 / 20) = 1103 lags
    with pytest.raises(ValueError, match='1024'):
        eng.f0(x, 22050, 275, tau_min=80, tau_max=70)
    for kw in (dict(hop_length=0), dict(hop_length=2.5), dict(window=0), dict(threshold=float('nan')), dict(fmin=0.0), dict(fmax=50.0),
               dict(n_samples=[5000, 0]), dict(n_samples=[5000, 5001]), dict(n_samples=[5000])):
        args = dict(dict(hop_length=275), **kw)
        with pytest.raises(ValueError):
            eng.f0(x, 22050, **args)
    with pytest.raises(ValueError):
        eng.f0(np.zeros((1, 2, 3), np.float32), 22050, 275)
    with pytest.raises(ValueError):
        eng.f0(x, float('nan'), 275)
    a, b, path = np.zeros((2, 40), np.float32), np.zeros((2, 55), np.float32), np.zeros((2, 94, 2), np.int32)
    for bad in ((a[0], b, path), (a, b[:1], path), (a, b, path[:, :, :1]), (a, b, path[:1]), (a, b, path[0])):
        with pytest.raises(ValueError):
            eng.f0_compare(*bad)
