"""GPU: the equaliser of synthesis (tts_set_equalizer).  With the setting on, a call is, bit for bit, the same call made without it
followed by tts_equalize on its rows -- behind the peak normalisation, with end-of-speech stopping (each utterance over the
hop (n[b] - 1) samples its row holds) and a pitch, ahead of the limiter and of the loudness gain, in the device and the host form
and with an encoded output.  With the setting off the call is the call as it was, and the stage counts no launch.
``synthesize_text`` equalises the joined rows.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations) at a power of 0.3 and
8 000 Hz, as tests/test_gpu_loudness_synth.py explains; the 'telephony' profile fits 8 000 Hz (3400 Hz is 0.425 of it)."""
import numpy as np
import pytest

import encode_cases as EC
import encode_oracle as EO
import eos_cases as E
import equalizer_cases as C
import equalizer_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
TARGET = (-23.0, 1e6)
UP = 4.0 / 12.0
POWER = 0.3
MS, L = 2.0, 16             # the limiter's look-ahead: 2 ms are 16 samples at 8 kHz
EQ = 'telephony'
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
        off = self.run(want_linear=True)              # on a handle whose equaliser was never touched
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None
        self.sos = O.profile(EQ, SR)

    def args(self):
        c = self.case
        return (self.ids, c['S'], E.REF_DB, E.MAX_DB, POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, peak=False, want_linear=False, **settings):
        return self.engine.synthesize(*self.args(), seed=SEED, peak_normalize=peak, want_linear=want_linear, **settings)

    def by_hand(self, peak=False, **settings):
        """the call without the equaliser, then tts_equalize on its rows -> (the device rows, their lengths or None)"""
        out = self.run(peak=peak, **settings)
        lens = self.hop * (out['n_frames'].astype(np.int32) - 1) if 'n_frames' in out else None
        return self.engine.equalize(out['wav'], EQ, n_samples=lens), lens


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def test_the_profile_the_engine_makes_is_the_oracles(case):
    H = pkg('_hip')
    np.testing.assert_allclose(H.equalizer_sections(H.equalizer_setting(EQ), SR), case.sos, rtol=1e-13, atol=0)
    x = case.off[0]
    d = case.engine.equalize(x, EQ)
    assert C.same(d.to_host(), O.equalize(x, H.equalizer_profile(EQ, SR)))
    d.free()


FORMS = dict(plain=dict(), peak=dict(peak=True), stopping=dict(stop_at_silence='own'), pitch=dict(pitch=UP, peak=True),
             everything=dict(pitch=UP, stop_at_silence='own', peak=True))


@pytest.mark.parametrize('form', sorted(FORMS))
def test_a_call_with_the_equaliser_is_the_call_then_the_equaliser(case, form):
    kw = dict(FORMS[form])
    if kw.get('stop_at_silence') == 'own':
        kw['stop_at_silence'] = (case.threshold_db, 0)
    rows, lens = case.by_hand(**kw)
    want = rows.to_host()
    assert not np.array_equal(bits(want), bits(case.run(**kw)['wav'].to_host()))
    if lens is not None:
        assert len(set(lens.tolist())) > 1
        for b, n in enumerate(lens):
            assert not want[b, n:].any()                                 # the zeros behind an utterance stay zeros
    got = case.run(equalizer=EQ, **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want)), form
    assert case.engine._equalizer is None                                # the scope put the handle's setting back
    # the host form: three calls in flight
    peak = kw.pop('peak', False)
    tickets = [case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=peak, equalizer=EQ, **kw) for _ in range(3)]
    for t in tickets:
        assert np.array_equal(bits(case.engine.wait_host(t)), bits(want)), form


@pytest.mark.parametrize('stopping', [False, True])
def test_the_limiter_and_the_loudness_gain_run_behind_the_equaliser(case, stopping):
    eng = case.engine
    kw = dict(stop_at_silence=(case.threshold_db, 0)) if stopping else {}
    # a limiter on top: the call without either, the equaliser, the limiter
    rows, lens = case.by_hand(peak=True, **kw)
    ceiling = float(np.abs(rows.to_host()).max()) / 3.0
    limited, stats = eng.limit(rows, ceiling, L, 4, n_samples=lens)
    want = limited.to_host()
    assert stats['over'].sum() > 0
    got = case.run(peak=True, equalizer=EQ, limiter=(ceiling, MS, 4), **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want))
    t = eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=True, equalizer=EQ, limiter=(ceiling, MS, 4), **kw)
    assert np.array_equal(bits(eng.wait_host(t)), bits(want))
    # a loudness target and no peak normalisation: the call without either, the equaliser, the loudness normalisation
    rows, lens = case.by_hand(peak=False, **kw)
    levelled, gains = eng.loudness_normalize(rows, SR, TARGET[0], TARGET[1], n_samples=lens)
    want = levelled.to_host()
    assert np.any(gains != 1.0)                                          # (a row cut under 400 ms keeps its level: gain 1)
    got = case.run(peak=False, equalizer=EQ, loudness=TARGET, **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want))
    t = eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=False, equalizer=EQ, loudness=TARGET, **kw)
    assert np.array_equal(bits(eng.wait_host(t)), bits(want))


def test_an_encoded_output_is_made_of_the_equalised_rows(case):
    rows, _lens = case.by_hand(peak=True)
    want, wst = EO.encode(rows.to_host(), EO.S16, EO.TPDF, SEED)
    codes, n_samples, stats = case.engine.wait_host_encoded(
        case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=True, equalizer=EQ, output='pcm16'))
    assert codes.dtype == np.int16 and EC.same_bits(codes, want) and n_samples.tolist() == [want.shape[1]] * case.B
    assert EC.same_records(stats, wst)


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again, or refused: the bits of the handle that never heard of the setting, and no launch in
    stage "equalize" """
    c, eng = case, case.engine
    H = pkg('_hip')
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('equalize') == (0.0, 0)
        on = c.run(equalizer=EQ)['wav'].to_host()
        assert eng.profile_get('equalize')[1] == 4                       # the transition and the three passes
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('equalize') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
    assert not np.array_equal(bits(on), bits(c.off))
    # the identity section: the setting on, and still the bits of the call as it was
    assert np.array_equal(bits(c.run(equalizer=np.array([[1.0, 0.0, 0.0, 0.0, 0.0]]))['wav'].to_host()), bits(c.off))
    # sections by design and as an array are the profile's
    design = [('highpass', 300.0, H.EQ_Q_BUTTER4[0]), ('highpass', 300.0, H.EQ_Q_BUTTER4[1]), ('lowpass', 3400.0, H.EQ_Q_BUTTER4[0]),
              ('lowpass', 3400.0, H.EQ_Q_BUTTER4[1])]
    assert np.array_equal(bits(c.run(equalizer=design)['wav'].to_host()), bits(on))
    assert np.array_equal(bits(c.run(equalizer=H.equalizer_profile(EQ, SR))['wav'].to_host()), bits(on))
    # the handle's setting, read when the call is made
    eng.set_equalizer(EQ)
    try:
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
        with pytest.raises(ValueError, match='bright'):
            eng.set_equalizer('bright')                                  # 6 kHz does not fit 8 kHz
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))  # refused settings leave the handle's as it was
        assert np.array_equal(bits(c.run(equalizer=np.array([[1.0, 0.0, 0.0, 0.0, 0.0]]))['wav'].to_host()), bits(c.off))
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
    finally:
        eng.set_equalizer(None)
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))


def test_synthesize_text_equalises_the_joined_rows():
    """on the texts of tests/test_gpu_long_text.py: every text is the equaliser's answer to the text without it (a row's result is
    the bits of its B = 1 call), ahead of the loudness gain where there is one"""
    import test_gpu_long_text as LT
    c = LT.Case()
    try:
        c.hp.magnitude_power, c.engine.sampling_rate = 0.3, SR          # (as that file's loudness test runs them)
        plain = LT.run(c)
        got = LT.run(c, equalizer=EQ)
        levelled = LT.run(c, equalizer=EQ, loudness=TARGET)
        assert [len(w) for w in got] == [len(w) for w in plain] == [len(w) for w in levelled]
        for g, w in enumerate(plain):
            want = c.engine.equalize(w, EQ)
            assert np.array_equal(bits(got[g]), bits(want.to_host())), g
            want, _gains = c.engine.loudness_normalize(want, SR, TARGET[0], TARGET[1])
            assert np.array_equal(bits(levelled[g]), bits(want.to_host())), g
            want.free()
        assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(got, plain))
    finally:
        c.engine.close()
