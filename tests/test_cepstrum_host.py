"""Cepstra and mel-cepstral distortion without a GPU: the float64 oracle (tests/cepstrum_oracle.py) against scipy's DCT, how far
above the kernel's error bound a wrong transform lies, the Python surface (audio.features.calculate_mfccs,
audio.metrics.mel_cepstral_distortion) on an engine whose two device calls are the oracles, the refusals of tts_mfcc and tts_dtw
-- which return before a device is touched -- and the exported symbols."""
import ctypes

import numpy as np
import pytest

import cepstrum_oracle as C
import dtw_cases as K
import dtw_oracle as W
from conftest import pkg
from host_checks import no_device_engine


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('n_mels', [1, 16, 80, 272, 1024])
def test_the_oracle_is_scipys_orthonormal_dct(n_mels):
    fft = pytest.importorskip('scipy.fftpack')
    rng = np.random.default_rng(n_mels)
    x = rng.random((2, 5, n_mels))
    y, _ = C.mfcc(x, n_mels)
    ref = fft.dct(x, type=2, norm='ortho', axis=-1)
    err = np.abs(y - ref).max()
    print('n_mels {}: max |oracle - scipy| = {:.2e}'.format(n_mels, err))
    assert err <= 1e-12
    d = C.dct_matrix(n_mels)
    assert np.abs(d @ d.T - np.eye(n_mels)).max() <= 1e-12   # orthonormal


def test_what_the_bound_tells_apart():
    """A transform that drops one term or misses the 1 / sqrt(2) of row 0 lies orders of magnitude above the bound
    2^-24 |y| + 2^-40 sum |d| |x|; the float32 rounding of the oracle itself lies inside it."""
    rng = np.random.default_rng(0)
    x = rng.random((1, 64, 80)).astype(np.float32)
    d = C.dct_matrix(80, 13)
    y, scale = C.mfcc(x, 13)
    assert C.within_bound(y.astype(np.float32), y, scale)
    dropped = d.copy()
    dropped[:, 79] = 0.0                      # the last term of every sum
    unscaled = d.copy()
    unscaled[0] *= np.sqrt(2.0)               # row 0 without its 1 / sqrt(2)
    for wrong, rows in ((dropped, slice(0, 13)), (unscaled, slice(0, 1))):
        z, _ = C.mfcc(x, 13, d=wrong)
        excess = (np.abs(z - y) / C.bound(y, scale))[..., rows]
        print('smallest excess over the bound: {:.1e}'.format(excess.min()))
        assert not C.within_bound(z.astype(np.float32), y, scale)
        assert np.median(excess) > 1e3
    # clip01 is np.clip: values outside [0, 1] change the result, a NaN stays
    x2 = x.copy()
    x2[0, 3, 5], x2[0, 4, 6], x2[0, 5, 7] = 1.5, -0.25, np.nan
    y2, _ = C.mfcc(x2, 13, clip01=True)
    assert np.isnan(y2[0, 5]).all() and not np.isnan(np.delete(y2, 5, axis=1)).any()
    x3 = x2.copy()
    x3[0, 3, 5], x3[0, 4, 6] = 1.0, 0.0
    assert np.array_equal(np.delete(C.mfcc(x3, 13)[0], 5, axis=1), np.delete(y2, 5, axis=1))


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
    """an engine whose mfcc and dtw are the numpy oracles: the layers above them run as they are"""

    def mfcc(self, rows, n_mfcc, n_frames=None, clip01=False, row_stride=None):
        rows = rows.a if isinstance(rows, _Host) else rows
        return _Host(C.mfcc(rows, n_mfcc, n_frames, clip01)[0].astype(np.float32))

    def dtw(self, a, b, n_a=None, n_b=None, D=None, want_path=False, skip=0):
        a, b = a.a, b.a
        B = a.shape[0]
        cost, plen = np.zeros(B), np.zeros(B, np.int32)
        path = np.full((B, a.shape[1] + b.shape[1] - 1, 2), -1, np.int32)
        for p in range(B):
            na = a.shape[1] if n_a is None else int(n_a[p])
            nb = b.shape[1] if n_b is None else int(n_b[p])
            cost[p], plen[p], pth = W.dtw_diagonals(a[p, :na, skip:], b[p, :nb, skip:], D)
            path[p, :len(pth)] = pth
        return (_Host(cost), _Host(plen), _Host(path)) if want_path else (_Host(cost), _Host(plen))


def test_calculate_mfccs_takes_the_reference_layout():
    F = pkg('audio.features')
    fft = pytest.importorskip('scipy.fftpack')
    rng = np.random.default_rng(1)
    mel_db = (100.0 * rng.random((80, 23)) - 100.0).astype(np.float32)   # (n_mels, t), in dB
    got = F.calculate_mfccs(mel_db, 22050, 13, engine=_OracleEngine())
    assert got.shape == (13, 23) and got.dtype == np.float32
    ref = fft.dct(mel_db.astype(np.float64), axis=0, type=2, norm='ortho')[:13]   # librosa.feature.mfcc(S=mel_db, n_mfcc=13)
    assert np.abs(got - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    with pytest.raises(ValueError):
        F.calculate_mfccs(mel_db[0], 22050, 13, engine=_OracleEngine())


def test_mel_cepstral_distortion_is_the_textbook_formula():
    """normalised-dB rows -> de-normalised dB -> natural-log cepstra -> (10 / ln 10) sqrt(2 sum dc^2), averaged along the path"""
    M = pkg('audio.metrics')
    ref_db, max_db, n = 6.02, 99.89, 13
    a, b = K.warped_pair(3, 30, 41, 80)
    mel_a = (0.5 + 0.2 * np.tanh(a)).astype(np.float32)
    mel_b = (0.5 + 0.2 * np.tanh(b)).astype(np.float32)
    mel_a[4, 7], mel_b[9, 3] = 1.25, -0.5        # outside [0, 1]: clipped, as the reference clips before it de-normalises
    n_a, n_b = np.array([27], np.int32), np.array([41], np.int32)
    out = M.mel_cepstral_distortion(mel_a[None], mel_b[None], n_a=n_a, n_b=n_b, n_coeffs=n, ref_db=ref_db, max_db=max_db,
                                    engine=_OracleEngine(), want_path=True)
    plen = int(out['path_len'][0])
    path = out['path'][0, :plen]
    assert (out['path'][0, plen:] == -1).all() and tuple(path[-1]) == (26, 40)
    # the textbook evaluation along that path
    d = C.dct_matrix(80, n + 1)

    def ln_cepstra(x):
        db = np.clip(x.astype(np.float64), 0, 1) * (abs(ref_db) + abs(max_db)) - abs(max_db) + ref_db   # inv_normalize_decibel
        ln_mag = db / 20.0 * np.log(10.0)                                                              # 20 log10 m = db
        return ln_mag @ d.T

    ca, cb = ln_cepstra(mel_a), ln_cepstra(mel_b)
    per_step = [10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum((ca[i, 1:] - cb[j, 1:]) ** 2)) for i, j in path]
    print('mcd {:.6f} dB, textbook {:.6f} dB over {} steps'.format(out['mcd'][0], np.mean(per_step), plen))
    assert abs(out['mcd'][0] - np.mean(per_step)) <= 1e-5 * np.mean(per_step)   # (the cepstra are rounded to float32 on the way)
    assert out['mcd'][0] == M.mcd_scale(ref_db, max_db) * out['cost'][0] / plen
    assert abs(M.mcd_scale(ref_db, max_db) - C.mcd_scale(ref_db, max_db)) <= 1e-12
    # a pair against itself: exactly 0 along the diagonal
    same = M.mel_cepstral_distortion(mel_a[None], mel_a[None].copy(), engine=_OracleEngine())
    assert same['mcd'][0] == 0.0 and same['path_len'][0] == 30
    for bad in (0, 80, 2.5):
        with pytest.raises(ValueError):
            M.mel_cepstral_distortion(mel_a[None], mel_b[None], n_coeffs=bad, engine=_OracleEngine())
    with pytest.raises(ValueError):
        M.mel_cepstral_distortion(mel_a, mel_b, engine=_OracleEngine())


def test_evaluate_command_line_parses_the_switches():
    E = pkg('tacotron.evaluate')
    import inspect
    sig = inspect.signature(E.evaluate)
    assert sig.parameters['mcd'].default is False and sig.parameters['mcd_coeffs'].default == 13
    assert sig.parameters['mcd_stop_at_silence'].default is None
    with pytest.raises(SystemExit):
        E.main(['--mcd-coeffs', '5', '--checkpoint-dir', '/nonexistent'])
    with pytest.raises(SystemExit):
        E.main(['--mcd-stop-at-silence', '-40', '--checkpoint-dir', '/nonexistent'])
    with pytest.raises(FileNotFoundError):   # legal switches get as far as the checkpoint listing
        E.main(['--mcd', '--mcd-coeffs', '5', '--mcd-stop-at-silence', '-40', '--checkpoint-dir', '/nonexistent'])


# ---------------------------------------------------------------------------------------------- the library, without a device
def test_symbols_are_exported():
    H = pkg('_hip')
    lib = H.load_library()
    for name in ('tts_mfcc', 'tts_dtw', 'tts_dtw_max_frames', 'tts_dtw_tile'):
        assert name in H.exported_symbols() and getattr(lib, name) is not None
    assert lib.tts_dtw_max_frames() >= 2048
    assert 1 <= lib.tts_dtw_tile() <= lib.tts_dtw_max_frames()


def _i32(values):
    arr = (ctypes.c_int32 * len(values))(*values)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)), arr


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal is made on the arguments alone, ahead of the handle: with a NULL handle (there is no device here) a bad call
    and a good one are both refused, but only the bad one with its own code and reason.  The pointers are never dereferenced."""
    H = pkg('_hip')
    lib = H.load_library()
    INV, UNS = H.TTS_ERR_INVALID, H.TTS_ERR_UNSUPPORTED
    p = 4096   # any aligned non-NULL address

    def why():
        return (lib.tts_last_error(None) or b'').decode()

    # tts_mfcc(h, spec, B, T, n_mels, row_stride, n_frames, n_mfcc, clip01, out)
    good = [p, 3, 12, 80, 80, None, 13, 1, p]
    for at, bad, word in [(0, None, 'NULL'), (8, None, 'NULL'), (1, 0, '>= 1'), (2, 0, '>= 1'), (3, 0, '>= 1'), (6, 0, '>= 1'),
                          (3, 1025, '1024'), (6, 81, 'n_mfcc > n_mels'), (4, 79, 'row_stride')]:
        args = list(good)
        args[at] = bad
        if at == 3 and bad == 1025:
            args[4] = 1025
        assert lib.tts_mfcc(None, *args) == INV and word in why() and why().startswith('mfcc: '), (at, bad, why())
    for lens in ([12, 0, 1], [12, 13, 1], [-1, 1, 1]):
        ptr, keep = _i32(lens)
        args = list(good)
        args[5] = ptr
        assert lib.tts_mfcc(None, *args) == INV and 'n_frames[' in why(), lens

    # tts_dtw(h, a, Ta, stride_a, n_a, b, Tb, stride_b, n_b, B, D, cost, path_len, path)
    good = [p, 12, 14, None, p, 20, 13, None, 3, 13, p, p, None]
    for at, bad, word in [(0, None, 'NULL'), (4, None, 'NULL'), (10, None, 'NULL'), (11, None, 'NULL'), (8, 0, '>= 1'), (1, 0, '>= 1'),
                          (5, -3, '>= 1'), (9, 0, '>= 1'), (2, 12, 'stride'), (6, 12, 'stride'), (10, p + 4, '8-byte')]:
        args = list(good)
        args[at] = bad
        assert lib.tts_dtw(None, *args) == INV and word in why() and why().startswith('dtw: '), (at, bad, why())
    for which, lens in ((3, [12, 0, 1]), (3, [13, 1, 1]), (7, [20, 21, 1]), (7, [1, 1, -2])):
        ptr, keep = _i32(lens)
        args = list(good)
        args[which] = ptr
        assert lib.tts_dtw(None, *args) == INV and ('n_a[' if which == 3 else 'n_b[') in why(), lens
    limit = lib.tts_dtw_max_frames()
    for at in (1, 5):
        args = list(good)
        args[at] = limit + 1
        assert lib.tts_dtw(None, *args) == UNS and str(limit) in why(), why()
    args = list(good)
    args[2] = args[6] = 200
    args[9] = 129
    assert lib.tts_dtw(None, *args) == UNS and '128' in why()
    # padding beyond the limit is legal while the lengths are not: what is left is the missing handle
    ptr, keep = _i32([limit, 3, 1])
    args = list(good)
    args[1], args[3] = limit + 50, ptr
    before = why()
    assert lib.tts_dtw(None, *args) == INV and why() == before
    assert lib.tts_mfcc(None, p, 3, 12, 80, 80, None, 13, 1, p) == INV and why() == before


def test_python_refuses_bad_arguments_before_any_device_call():
    eng = no_device_engine()
    rows = np.ones((3, 12, 80), np.float32)
    for n_mfcc in (0, 81, 2.5):
        with pytest.raises(ValueError):
            eng.mfcc(rows, n_mfcc)
    with pytest.raises(ValueError):
        eng.mfcc(rows[0], 13)
    with pytest.raises(ValueError):
        eng.mfcc(rows, 13, row_stride=79)
    for bad in ([12, 0, 1], [12, 13, 1], [12, 1], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            eng.mfcc(rows, 13, n_frames=bad)
    a, b = np.ones((3, 12, 14), np.float32), np.ones((3, 20, 14), np.float32)
    with pytest.raises(ValueError):
        eng.dtw(a, b[:2])
    with pytest.raises(ValueError):
        eng.dtw(a[0], b[0])
    for D, skip in ((0, 0), (15, 0), (14, 1), (1.5, 0), (1, -1)):
        with pytest.raises(ValueError):
            eng.dtw(a, b, D=D, skip=skip)
    with pytest.raises(ValueError):
        eng.dtw(a, b, n_a=[12, 13, 1])
    with pytest.raises(ValueError):
        eng.dtw(a, b, n_b=[20, 0, 1])
