"""GPU parity of the analysis kernels per slice: tts_stft, tts_stft_magnitude and tts_mel_spectrogram against the float64
oracle (A.stft(..., dtype=complex128), not its complex64 default) on every axis -- utterance, bin / channel, frame,
element -- at 1e-5, over the tables of audio_cases.py (test_audio_bounds_host.py shows float32 arithmetic within a quarter
of that bound on these inputs).

One rel-L2 over the matrix dilutes exactly what the two STFT kernels special-case: the Nyquist bin has a line of its own
(stft_kernel: orow[MH]; glg_stft_kernel: k == M), the half-size transform is untangled with a twiddle table, the first and
last frames reflect the signal with two index lines, and the utterance offset is b * n.  Here both kernels (n_fft 2048 and
the general ones at 256 ... 4096, an odd window among them) see B = 1, 3 and 9 different signals, the shortest legal length
(n_fft / 2 + 1: every frame reflected on both sides), lengths = 1 and = hop - 1 (mod hop), lengths below n_fft and 3001
frames at hop 50.
"""
import numpy as np
import pytest

import audio_cases as C
from conftest import pkg
from oracle import audio_oracle as A
from parity import assert_parity

pytestmark = pytest.mark.gpu
TOL = C.ANALYSIS_TOL


@pytest.mark.parametrize('kind', sorted(C.SIGNALS))
@pytest.mark.parametrize('case', range(len(C.ANALYSIS_CASES)))
def test_stft_magnitude_and_mel_per_slice(engine, case, kind):
    n_fft, win, hop, n, B = C.ANALYSIS_CASES[case]
    y = C.signals(kind, case, B, n)
    ref = C.ref_stft(y, n_fft, win, hop)
    label = '{} case {} {}'.format(kind, case, C.ANALYSIS_CASES[case])
    d_y = engine.to_device(y)
    S = engine.stft(d_y, n_fft, win, hop).to_host()
    assert S.dtype == np.complex64 and S.shape == ref.shape == (B, 1 + n_fft // 2, 1 + n // hop)
    assert_parity(C.as_real(S), C.as_real(ref), C.STFT_AXES, TOL, label + ' stft')
    lin = None
    for p in C.POWERS:
        m = engine.stft_magnitude(d_y, n_fft, win, hop, p)
        assert_parity(m.to_host(), np.abs(ref) ** p, C.STFT_AXES, TOL, label + ' |S|^{}'.format(p))
        lin = lin if lin is not None else m
    sr, _, n_mels, fmin, fmax = C.MEL_CONFIGS[0]
    mel = engine.mel_spectrogram(lin, n_fft, sr, n_mels, fmin, fmax).to_host()
    rmel = np.matmul(A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax), np.abs(ref))
    assert_parity(mel, rmel, C.MEL_AXES, TOL, label + ' mel')


@pytest.mark.parametrize('n_fft,win,hop', C.STFT_CONFIGS)
def test_stft_refuses_half_a_transform_of_signal(engine, n_fft, win, hop):
    """n = n_fft / 2 + 1 is the shortest legal length (covered above); n = n_fft / 2 has no reflect padding"""
    y = C.signals('tone', 1, 2, n_fft // 2)
    for call in (lambda: engine.stft(y, n_fft, win, hop), lambda: engine.stft_magnitude(y, n_fft, win, hop, 1.0)):
        with pytest.raises(pkg().TtsError) as e:
            call()
        assert e.value.code == -1   # TTS_ERR_INVALID


@pytest.mark.parametrize('n_fft,a,b', [(2048, (1102, 275), (800, 200)), (2048, (1103, 275), (2048, 512)),
                                       (1024, (800, 200), (1024, 256)), (512, (400, 100), (401, 100))])
def test_stft_window_cache_a_b_a(engine, n_fft, a, b):
    """the handle caches one window table per path: window A, then B, then A again gives the bits of the first call, and B's
    result is B's (not A's table under B's arguments)"""
    y = C.signals('broadband', 5, 3, 9001)
    first = engine.stft(y, n_fft, a[0], a[1]).to_host()
    other = engine.stft(y, n_fft, b[0], b[1]).to_host()
    again = engine.stft(y, n_fft, a[0], a[1]).to_host()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    assert_parity(C.as_real(other), C.as_real(C.ref_stft(y, n_fft, b[0], b[1])), C.STFT_AXES, TOL,
                  'window cache {} B={}'.format(n_fft, b))
    assert_parity(C.as_real(again), C.as_real(C.ref_stft(y, n_fft, a[0], a[1])), C.STFT_AXES, TOL,
                  'window cache {} A={}'.format(n_fft, a))


@pytest.mark.parametrize('B', C.MEL_BATCHES)
@pytest.mark.parametrize('n_frames', C.MEL_FRAMES)
@pytest.mark.parametrize('cfg', range(len(C.MEL_CONFIGS)))
def test_mel_per_slice(engine, cfg, n_frames, B):
    sr, n_fft, n_mels, fmin, fmax = C.MEL_CONFIGS[cfg]
    lin = C.mel_input(cfg, n_frames, B)
    ref = np.matmul(A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax), lin.astype(np.float64))
    got = engine.mel_spectrogram(lin, n_fft, sr, n_mels, fmin, fmax).to_host()
    assert got.shape == ref.shape == (B, n_mels, n_frames)
    assert_parity(got, ref, C.MEL_AXES, TOL, 'mel cfg {} frames {} B {}'.format(cfg, n_frames, B))


@pytest.mark.parametrize('cfg', range(len(C.MEL_CONFIGS)))
def test_mel_filter_bank_entry_by_entry(engine, cfg):
    """lin = I (F frames, frame t one-hot in bin t): the output IS the filter bank -- 1.0 times a weight is exact under the
    three-way bf16 split, every other product is an exact zero -- so every entry is held to 1e-6 of the bank's maximum
    (float32 storage of the float64 bank is 6e-8 relative): one filter scaled by 1.001, a shifted edge or a wrong
    normalisation cannot hide behind the spectrum's shape."""
    sr, n_fft, n_mels, fmin, fmax = C.MEL_CONFIGS[cfg]
    F = 1 + n_fft // 2
    bank = A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    got = engine.mel_spectrogram(np.eye(F, dtype=np.float32)[None], n_fft, sr, n_mels, fmin, fmax).to_host()[0]
    assert got.shape == bank.shape == (n_mels, F)
    err = np.abs(got.astype(np.float64) - bank)
    m, f = np.unravel_index(int(np.argmax(err)), err.shape)
    print('mel bank cfg {}: worst entry {:.3e} of the maximum at filter {} bin {}'.format(cfg, err[m, f] / bank.max(), m, f))
    assert err.max() <= 1e-6 * bank.max(), (cfg, m, f, got[m, f], bank[m, f])


def test_mel_filter_bank_cache_a_b_a(engine):
    (sa, na, ma, la, ha), (sb, nb, mb, lb, hb) = C.MEL_CONFIGS[0], C.MEL_CONFIGS[1]
    lin_a, lin_b = C.mel_input(0, 33, 3), C.mel_input(1, 33, 3)
    first = engine.mel_spectrogram(lin_a, na, sa, ma, la, ha).to_host()
    other = engine.mel_spectrogram(lin_b, nb, sb, mb, lb, hb).to_host()
    again = engine.mel_spectrogram(lin_a, na, sa, ma, la, ha).to_host()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    ref_b = np.matmul(A.mel_filterbank(sb, nb, mb, lb, hb), lin_b.astype(np.float64))
    assert_parity(other, ref_b, C.MEL_AXES, TOL, 'mel cache B')
    # the same n_fft and channel count, another band: the bank is rebuilt, not reused
    band = engine.mel_spectrogram(lin_a, na, sa, ma, 50.0, 7600.0).to_host()
    ref_band = np.matmul(A.mel_filterbank(sa, na, ma, 50.0, 7600.0), lin_a.astype(np.float64))
    assert_parity(band, ref_band, C.MEL_AXES, TOL, 'mel cache band')
