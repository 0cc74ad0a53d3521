"""GPU: the limiter of synthesis (tts_set_limiter).  With the setting on, a call is, bit for bit, the same call made without it
followed by tts_limit on its rows -- behind the peak normalisation, behind the loudness gain, with end-of-speech stopping (each
utterance over the hop (n[b] - 1) samples its row holds) and a pitch, in the device and the host form.  With the setting off the
call is the call as it was, and the stage counts no launch.  ``synthesize_text`` limits the joined rows.  And what the limiter is
for: a row whose loudness gain would clip comes out at its target.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations) at a power of 0.3 and
8 000 Hz, as tests/test_gpu_loudness_synth.py explains.  The synthetic network's waveforms have no particular level, so every
ceiling here is taken from the rows it is to bind on: a third of their peak."""
import numpy as np
import pytest

import eos_cases as E
import limiter_cases as C
import limiter_oracle as O
import loudness_oracle as LO
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
TARGET = (-23.0, 1e6)
UP = 4.0 / 12.0
POWER = 0.3
MS, L = 2.0, 16             # the look-ahead: 2 ms are 16 samples at 8 kHz
bits = C.bits


class Case(object):
    def __init__(self, case):
        self.case = case
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.sampling_rate = SR
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.hop = case['B'], case['hop']
        off = self.run(want_linear=True)              # on a handle whose limiter was never touched
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None

    def args(self):
        c = self.case
        return (self.ids, c['S'], E.REF_DB, E.MAX_DB, POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, peak=False, want_linear=False, **settings):
        return self.engine.synthesize(*self.args(), seed=SEED, peak_normalize=peak, want_linear=want_linear, **settings)

    def by_hand(self, oversample, peak=False, **settings):
        """the call without the limiter, then tts_limit at a third of its peak on the rows -> (waveforms, limiter, stats)"""
        out = self.run(peak=peak, **settings)
        lens = self.hop * (out['n_frames'].astype(np.int32) - 1) if 'n_frames' in out else None
        ceiling = float(np.abs(out['wav'].to_host()).max()) / 3.0
        wav, stats = self.engine.limit(out['wav'], ceiling, L, oversample, n_samples=lens)
        return wav.to_host(), (ceiling, MS, oversample), stats, lens


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


FORMS = dict(plain=dict(), peak=dict(peak=True), loudness=dict(loudness=TARGET),
             everything=dict(loudness=TARGET, pitch=UP, stop_at_silence='own'))


@pytest.mark.parametrize('oversample', [1, 4])
@pytest.mark.parametrize('form', sorted(FORMS))
def test_a_call_with_the_limiter_is_the_call_then_the_limiter(case, form, oversample):
    kw = dict(FORMS[form])
    if kw.get('stop_at_silence') == 'own':
        kw['stop_at_silence'] = (case.threshold_db, 0)
    want, limiter, stats, lens = case.by_hand(oversample, **kw)
    assert stats['over'].sum() > 0 and np.all(stats['limited'] >= stats['over']) and stats['min_gain'].min() < 1.0, stats
    assert np.abs(want).max() <= O.ceiling_float(limiter[0])
    if lens is not None:
        assert len(set(lens.tolist())) > 1
        for b, n in enumerate(lens):
            assert not want[b, n:].any()                                 # the zeros behind an utterance stay zeros
    got = case.run(limiter=limiter, **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want)), form
    assert case.engine._limiter is None                                  # the scope put the handle's setting back
    # the host form: three calls in flight
    peak = kw.pop('peak', False)
    tickets = [case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=peak, limiter=limiter, **kw) for _ in range(3)]
    for t in tickets:
        assert np.array_equal(bits(case.engine.wait_host(t)), bits(want)), form


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again, or refused: the bits of the handle that never heard of the setting, and no launch in
    stage "limiter" """
    c, eng = case, case.engine
    H = pkg('_hip')
    limiter = (float(np.abs(c.off).max()) / 3.0, MS, 4)
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('limiter') == (0.0, 0)
        on = c.run(limiter=limiter)['wav'].to_host()
        assert eng.profile_get('limiter')[1] == 4                        # a fill and three kernels
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('limiter') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
    assert not np.array_equal(bits(on), bits(c.off))
    # a ceiling above every sample: the setting on, and still the bits of the call as it was
    assert np.array_equal(bits(c.run(limiter=(float(np.abs(c.off).max()), MS, 1))['wav'].to_host()), bits(c.off))
    # the handle's setting, read when the call is made
    eng.set_limiter(limiter)
    try:
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
        for bad in ((0.0, L, 4), (float('nan'), L, 4), (float('inf'), L, 4), (-1.0, L, 4), (0.5, -1, 4), (0.5, 1025, 4), (0.5, L, 2)):
            assert eng.lib.tts_set_limiter(eng.handle, 1, bad[0], bad[1], bad[2]) == H.TTS_ERR_INVALID, bad
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))  # refused settings leave the handle's as it was
    finally:
        eng.set_limiter(None)
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))


def test_synthesize_text_limits_the_joined_rows():
    """on the texts of tests/test_gpu_long_text.py: every text is the limiter's answer to the text without it (a row's result is
    the bits of its B = 1 call), behind the loudness gain where there is one"""
    import test_gpu_long_text as LT
    c = LT.Case()
    try:
        c.hp.magnitude_power, c.engine.sampling_rate = 0.3, SR          # (as that file's loudness test runs them)
        for settings in (dict(), dict(loudness=TARGET)):
            plain = LT.run(c, **settings)
            ceiling = float(max(np.abs(w).max() for w in plain)) / 3.0
            got = LT.run(c, limiter=(ceiling, MS, 4), **settings)
            assert [len(w) for w in got] == [len(w) for w in plain]
            for g, w in enumerate(plain):
                want, _stats = c.engine.limit(w, ceiling, L, 4)
                assert np.array_equal(bits(got[g]), bits(want.to_host())), (g, settings)
                want.free()
                assert np.abs(got[g]).max() <= O.ceiling_float(ceiling)
            assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(got, plain))
    finally:
        c.engine.close()


def test_a_row_whose_loudness_gain_would_clip_comes_out_at_the_target(engine):
    """Four seconds of speech-like noise at -20 LUFS with one plosive at 1.5, taken to -16 LUFS under a ceiling of 0.9: one gain
    under the ceiling leaves the row 8 dB short of the target; with head room for the gain and the limiter behind it the row is at
    the target (the plosive held 0.7 % of the energy) and under the ceiling.  The chain's loudness is held against the oracles' run of the same chain (tests/loudness_oracle.py,
    tests/limiter_oracle.py) within 1e-9 of the mean square, the bound the loudness oracle is held to its plain restatement
    with."""
    H = pkg('_hip')
    n, target, ceiling = 4 * SR, -16.0, 0.9
    x = C.speech_like(n, 0.4)
    x[9000] = 1.5
    k, taps = H.loudness_filter(SR), H.true_peak_filter()
    # one gain, capped at the ceiling
    capped, gains = engine.loudness_normalize(x, SR, target, ceiling)
    short = float(engine.loudness(capped, SR)[0])
    capped.free()
    assert gains[0] == ceiling / 1.5 and short < target - 6.0
    # the chain: head room of 4.0 for the gain, then the limiter
    work, gains, z = engine.loudness_normalize(x, SR, target, 4.0, return_mean_square=True)
    work, stats = engine.limit(work, ceiling, L, 1)
    got = work.to_host()
    lufs, z_got = engine.loudness(work, SR, return_mean_square=True)
    work.free()
    assert 1 <= stats['over'][0] < 10 and stats['over'][0] <= stats['limited'][0] <= stats['over'][0] * (4 * L + 1)
    assert np.abs(got).max() <= O.ceiling_float(ceiling)
    assert abs(float(lufs[0]) - target) < 0.1, lufs               # (the limiter took a few dozen of 32 000 samples down)
    # the oracles' run of the same chain
    z_x = LO.mean_square(x, SR, k)[0]
    assert np.float64(z_x) == z[0]
    g = LO.gain(z_x, LO.finite_peak(x), target, 4.0)
    scaled = (np.float64(g) * x.astype(np.float64)).astype(np.float32)
    want, _stats = O.limit(scaled, taps, ceiling, L, 1)
    z_want = LO.mean_square(want, SR, k)[0]
    assert abs(float(z_got[0]) - z_want) <= 1e-9 * z_want, (float(z_got[0]), z_want)
