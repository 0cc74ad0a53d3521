"""GPU: does the tone come out at the pitch asked for?  tts_f0 on what the resampler, Griffin-Lim and Engine.pitch_shift make of
harmonic tones of known pitch -- the first tests of those paths that listen to the result instead of checking their arithmetic.
The bounds come from the tracker's own measured error on such tones (tests/test_f0_host.py: 2.3e-4 relative at worst) and from
the float64 oracle chains, as stated at each check."""
import numpy as np
import pytest

import f0_cases as K
import f0_oracle as Y
import resample_oracle as R
import stretch_oracle as S
from oracle import audio_oracle as A

pytestmark = pytest.mark.gpu
E = K.EVAL
HOPS = 60
N = HOPS * E['hop']


def _track(engine, wav):
    """(n,) host or device waveform -> host f0 (T,)"""
    f0 = engine.f0(wav, K.SR, E['hop'], window=E['W'], tau_min=E['tau_min'], tau_max=E['tau_max'])
    out = f0.to_host().copy().reshape(-1)
    f0.free()
    return out


def _interior(T, n):
    half = (E['W'] + E['tau_max']) // 2
    return np.array([t for t in range(T) if t * E['hop'] - half >= 0 and t * E['hop'] - half + E['W'] + E['tau_max'] <= n])


def _voiced_median(f0):
    v = f0[f0 > 0]
    assert v.size >= f0.size // 2
    return float(np.median(v.astype(np.float64)))


@pytest.mark.parametrize('hz,s', [(150.0, 4), (220.0, -5), (110.0, 7)])
def test_the_resampler_moves_the_pitch(engine, hz, s):
    """a tone resampled by 2 ** (-s / 12) and heard at the old rate is s semitones higher: the median voiced f0 moves by
    2 ** (s / 12) within 1e-3, twice the sum of the tracker's worst errors on the two tones (2 * (2.3e-4 + 2.3e-4), rounded up)"""
    x = K.tone(hz, N, seed=int(hz))
    before = _voiced_median(_track(engine, x))
    y = engine.resample(x, 2.0 ** (-s / 12.0))
    after = _voiced_median(_track(engine, y))
    y.free()
    ratio = after / before
    print('{} Hz by {:+d} semitones: {:.3f} -> {:.3f} Hz, ratio off by {:.2e}'.format(hz, s, before, after, abs(ratio / 2.0 ** (s / 12.0) - 1.0)))
    assert abs(ratio / 2.0 ** (s / 12.0) - 1.0) <= 1e-3


@pytest.fixture(scope='module')
def tone210():
    return K.tone(210.0, N, seed=210)


def _deviation(f0, ref, inner):
    """(voiced share of the interior frames, median relative deviation of the voiced ones from ref)"""
    f = f0[inner].astype(np.float64)
    r = np.broadcast_to(np.asarray(ref, np.float64), f0.shape)[inner]
    voiced = f > 0
    return float(voiced.mean()), float(np.median(np.abs(f[voiced] / r[voiced] - 1.0))) if voiced.any() else float('inf')


def test_griffin_lim_keeps_the_pitch(engine, tone210):
    """|STFT| of a 210 Hz tone -> Griffin-Lim (30 iterations, random start) -> tts_f0 against the tone's own track: at least
    0.9 of the interior frames voiced and a median relative deviation of at most 5e-3 -- the float64 oracle chain gives 1.0 and
    1.1e-3, so the margin for the random start is about 4x"""
    own = _track(engine, tone210)
    mag = engine.stft_magnitude(tone210[None], 2048, 1102, 275, 1.0)
    wav, _ = engine.griffin_lim(mag, 30, 1102, 275, 2048, seed=5, want_mse=False, momentum=0.0, phase_init='random')
    f0 = _track(engine, wav)
    mag.free()
    wav.free()
    inner = _interior(f0.size, N)
    assert f0.size == HOPS + 1 and (own[inner] > 0).all()
    share, dev = _deviation(f0, own, inner)
    print('Griffin-Lim: {:.3f} of {} interior frames voiced, median relative deviation {:.2e}'.format(share, inner.size, dev))
    assert share >= 0.9 and dev <= 5e-3


def oracle_pitch_shift(x, octaves, n_iter=25, seed=0):
    """Engine.pitch_shift on the CPU: |STFT| (1024 / 1024 / 256), the stretch oracle at 2 ** -octaves, the Griffin-Lim of
    oracle/audio_oracle.py from random phases, the resample oracle back to the input's length"""
    rate = float(np.exp2(-np.float64(octaves)))
    mag = np.abs(A.stft(x, 1024, 256, 1024))
    st = S.blend(mag, rate)
    wav, _ = A.griffin_lim_v2(st, 1024, 256, 1024, n_iter, rng=np.random.default_rng(seed))
    y, _ = R.resample(wav, rate, n_out=x.shape[0])
    return y.astype(np.float32)


def test_pitch_shift_raises_the_pitch_by_four_semitones(engine, tone210):
    """Engine.pitch_shift of the 210 Hz tone by +4 semitones against 210 * 2 ** (4 / 12) Hz: the median relative deviation over the
    interior frames is held to four times what the CPU oracle chain gives (the same statistic, through tests/f0_oracle.py), the
    margin the Griffin-Lim check leaves for a random start, and at least 0.9 of the interior frames are voiced.
    DESIGN.md 4.11 records both figures."""
    want = 210.0 * 2.0 ** (4.0 / 12.0)
    inner = _interior(HOPS + 1, N)
    cpu = oracle_pitch_shift(tone210, 4.0 / 12.0)
    cpu_f0 = Y.f0(cpu[None], K.SR, E['hop'], E['W'], E['tau_min'], E['tau_max'], 0.1)[0][0]
    cpu_share, cpu_dev = _deviation(cpu_f0, want, inner)
    y = engine.pitch_shift(tone210, K.SR, 4.0 / 12.0, seed=3)
    assert y.shape == (N,)
    f0 = _track(engine, y)
    y.free()
    share, dev = _deviation(f0, want, inner)
    print('pitch_shift +4 semitones: oracle chain {:.3f} voiced, deviation {:.3e}; device {:.3f} voiced, deviation {:.3e}'.format(
        cpu_share, cpu_dev, share, dev))
    assert cpu_share >= 0.9 and share >= 0.9
    assert dev <= 4.0 * cpu_dev
