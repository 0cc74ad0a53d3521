"""The listening test of the formant-preserving pitch (a plain helper module): a 150 Hz tone of 60 hops at +4 semitones, once
through the device (``Engine.pitch_shift(.., preserve_formants=True)``, tracked by ``Engine.f0``) and once through the CPU oracles
(the STFT and the Griffin-Lim of oracle/audio_oracle.py around tests/shift_oracle.py, tracked by tests/f0_oracle.py), from the
same initial phases and with the same iterations.  Each gives the ratio of the median voiced F0 to the tracker's reading of the
input."""
import numpy as np

import f0_cases as K
import f0_oracle as FO
import shift_oracle as O
from oracle import audio_oracle as A

HZ, SEMITONES, N_ITER, SEED = 150.0, 4.0, 25, 7
N_FFT, WIN, HOP = 1024, 1024, 256
E = K.EVAL
O_ORDER = max(8, int(0.0015 * K.SR))   # 33: the default order at 22 050 Hz


def _tone():
    return K.tone(HZ, 60 * E['hop'], seed=150).astype(np.float32)


def _phases():
    n = _tone().shape[0]
    return np.random.default_rng(SEED).random((1, N_FFT // 2 + 1, 1 + n // HOP)).astype(np.float32)


def _median(f0):
    f0 = np.asarray(f0).reshape(-1)
    v = f0[f0 > 0]
    assert v.size >= max(1, f0.size // 2)
    return float(np.median(v.astype(np.float64)))


def device_ratio(engine):
    x = _tone()

    def track(wav):
        f0 = engine.f0(wav, K.SR, E['hop'], window=E['W'], tau_min=E['tau_min'], tau_max=E['tau_max'])
        out = f0.to_host().copy()
        f0.free()
        return _median(out)

    y = engine.pitch_shift(x, K.SR, SEMITONES / 12.0, n_iter=N_ITER, preserve_formants=True, order=O_ORDER, init_phase=_phases())
    try:
        host = y.to_host()
    finally:
        y.free()
    assert host.shape == x.shape and np.isfinite(host).all()
    return track(host) / track(x)



def oracle_ratio():
    x = _tone()
    mag = np.abs(A.stft(x, N_FFT, HOP, WIN)).astype(np.float32)[None]                 # (1, 513, 65)
    T = mag.shape[2]
    shifted = O.shift(mag, [(0, 0, T, O.step(SEMITONES), O.UNITY)], None, O_ORDER)['out']
    wav, _mse = A.griffin_lim_v2(shifted[0], WIN, HOP, N_FFT, N_ITER, init_phase=_phases()[0])
    y = np.zeros_like(x)
    y[:wav.shape[0]] = wav.astype(np.float32)

    def track(w):
        f0, _ap = FO.f0(w[None], K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)
        return _median(f0)

    return track(y) / track(x)
