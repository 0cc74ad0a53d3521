"""GPU: the loudness of synthesis (tts_set_loudness).  With a target, a call is, bit for bit, the same call made with
peak_normalize off followed by tts_loudness_normalize on its rows -- plain, with end-of-speech stopping (each utterance over the
hop (n[b] - 1) samples its row holds), with a pitch (behind the resampler) and in the host form -- whatever peak_normalize says.
With the setting off the call is the call as it was.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations).  The rows hold 10 725
samples, so the target is measured at 8 000 Hz here (13 steps, 10 blocks; at 22 050 Hz a row would be one block and a stopped
utterance none).  The synthetic network's spectrograms lie some 100 dB down -- at the reference's power of 1.3 its waveforms have
an rms of 3e-7 and never reach the absolute gate -- so the calls here use a power of 0.3, which lifts them above it."""
import numpy as np
import pytest

import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
TARGET = (-23.0, 1e6)       # (a ceiling that does not bind: the synthetic network's waveforms have no particular level)
UP = 4.0 / 12.0
POWER = 0.3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(object):
    def __init__(self, case):
        self.case = case
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.sampling_rate = SR
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.T, self.hop = case['B'], case['S'] * self.hp.reduction, case['hop']
        off = self.run(want_linear=True)              # on a handle whose loudness was never touched
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None
        self.stop = (self.threshold_db, 0)

    def args(self):
        c = self.case
        return (self.ids, c['S'], E.REF_DB, E.MAX_DB, POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, loudness=None, pitch=None, stop=None, peak=False, want_linear=False):
        return self.engine.synthesize(*self.args(), seed=SEED, peak_normalize=peak, want_linear=want_linear, stop_at_silence=stop,
                                      pitch=pitch, loudness=loudness)

    def by_hand(self, target, **kw):
        """the call with peak_normalize off, then tts_loudness_normalize on its rows -> (waveforms, gains)"""
        out = self.run(peak=False, **kw)
        lens = self.hop * (out['n_frames'].astype(np.int32) - 1) if 'n_frames' in out else None
        wav, gains = self.engine.loudness_normalize(out['wav'], SR, target[0], target[1], n_samples=lens)
        return wav.to_host(), gains, lens


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


@pytest.mark.parametrize('form', ['plain', 'stopping', 'pitch'])
def test_a_call_with_a_target_is_the_call_then_the_normaliser(case, form):
    kw = dict(plain={}, stopping=dict(stop=case.stop), pitch=dict(pitch=UP))[form]
    want, gains, lens = case.by_hand(TARGET, **kw)
    held = lens if lens is not None else np.full(case.B, want.shape[1])
    measured = held >= 4 * (SR // 10)                                     # (a stopped utterance may be shorter than a block)
    assert np.all(np.isfinite(gains)) and np.all(gains[measured] != 1.0) and np.all(gains[~measured] == 1.0) and measured.any(), \
        (gains, held, np.abs(want).max(axis=1))
    if form == 'stopping':
        assert len(set(lens.tolist())) > 1 and lens.max() <= want.shape[1]
        for b, n in enumerate(lens):
            assert not want[b, n:].any()                                 # the zeros behind an utterance stay zeros
    for peak in (True, False):                                            # peak_normalize is not applied either way
        got = case.run(loudness=TARGET, peak=peak, **kw)['wav'].to_host()
        assert np.array_equal(bits(got), bits(want)), (form, peak)
    assert case.engine._loudness is None                                  # the scope put the handle's setting back
    # every utterance reads the target over the samples it holds
    back = case.engine.loudness(want, SR, n_samples=lens)
    assert np.all(np.abs(back[measured] - TARGET[0]) < 1e-4), back
    # a ceiling that binds: the same composition
    tight = (TARGET[0], float(np.abs(want).max()) / 4.0)
    want_t, gains_t, _ = case.by_hand(tight, **kw)
    assert np.abs(want_t).max() <= tight[1] and np.any(gains_t < gains)
    assert np.array_equal(bits(case.run(loudness=tight, **kw)['wav'].to_host()), bits(want_t))


def test_the_host_form_is_the_device_form(case):
    eng = case.engine
    want = case.run(loudness=TARGET)['wav'].to_host()
    tickets = [eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=True, loudness=TARGET) for _ in range(3)]
    for t in tickets:
        assert np.array_equal(bits(eng.wait_host(t)), bits(want))
    t = eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=False)
    assert np.array_equal(bits(eng.wait_host(t)), bits(case.off))


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again, or refused: the bits of the handle that never heard of the setting, and no launch
    in stage "loudness" """
    c, eng = case, case.engine
    H = pkg('_hip')
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('loudness') == (0.0, 0)
        c.run(loudness=TARGET)
        assert eng.profile_get('loudness')[1] == 8                       # a fill and seven kernels
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('loudness') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
    # the handle's setting, read when the call is made
    on = c.run(loudness=TARGET)['wav'].to_host()
    assert not np.array_equal(bits(on), bits(c.off))
    eng.set_loudness(TARGET)
    try:
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
        # refused settings leave the handle's as it was
        for bad, code in (((float('nan'), 1.0, SR), H.TTS_ERR_INVALID), ((float('inf'), 1.0, SR), H.TTS_ERR_INVALID),
                          ((-23.0, 0.0, SR), H.TTS_ERR_INVALID), ((-23.0, -1.0, SR), H.TTS_ERR_INVALID),
                          ((-23.0, float('inf'), SR), H.TTS_ERR_INVALID), ((-23.0, float('nan'), SR), H.TTS_ERR_INVALID),
                          ((-23.0, 1.0, 7999), H.TTS_ERR_UNSUPPORTED), ((-23.0, 1.0, 192001), H.TTS_ERR_UNSUPPORTED)):
            assert eng.lib.tts_set_loudness(eng.handle, 1, bad[0], bad[1], bad[2]) == code, bad
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
    finally:
        eng.set_loudness(None)
    assert eng.lib.tts_set_loudness(None, 0, 0.0, 1.0, 0) == H.TTS_ERR_INVALID
    assert np.array_equal(bits(c.run(peak=True)['wav'].to_host()), bits(eng.peak_normalize(eng.to_device(c.off)).to_host()))
