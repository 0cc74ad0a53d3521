"""GPU: the compressor of synthesis (tts_set_compressor).  With the setting on, a call is, bit for bit, the same call made without it
followed by tts_compress on its rows -- behind the peak normalisation and the equaliser, with end-of-speech stopping (each
utterance over the hop (n[b] - 1) samples its row holds) and a pitch, ahead of the loudness gain and of the limiter, in the device
and the host form and with an encoded output.  With the setting off the call is the call as it was, and the stage counts no
launch.  ``synthesize_text`` compresses the joined rows.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations) at a power of 0.3 and
8 000 Hz, as tests/test_gpu_loudness_synth.py explains.  The 'speech' profile has a make-up gain, so it changes every sample."""
import numpy as np
import pytest

import compressor_cases as C
import compressor_oracle as O
import encode_cases as EC
import encode_oracle as EO
import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
TARGET = (-23.0, 1e6)
UP = 4.0 / 12.0
POWER = 0.3
MS, L = 2.0, 16             # the limiter's look-ahead: 2 ms are 16 samples at 8 kHz
CMP = 'speech'
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
        off = self.run(want_linear=True)              # on a handle whose compressor was never touched
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None

    def args(self):
        c = self.case
        return (self.ids, c['S'], E.REF_DB, E.MAX_DB, POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, peak=False, want_linear=False, **settings):
        return self.engine.synthesize(*self.args(), seed=SEED, peak_normalize=peak, want_linear=want_linear, **settings)

    def by_hand(self, peak=False, **settings):
        """the call without the compressor, then tts_compress on its rows -> (the device rows, their lengths or None)"""
        out = self.run(peak=peak, **settings)
        lens = self.hop * (out['n_frames'].astype(np.int32) - 1) if 'n_frames' in out else None
        return self.engine.compress(out['wav'], CMP, n_samples=lens), lens


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def test_the_profile_the_engine_makes_is_the_oracles(case):
    H = pkg('_hip')
    assert tuple(H.compressor_params(H.compressor_setting(CMP), SR)) == tuple(O.profile(CMP, SR))
    x = case.off[0] / np.abs(case.off[0]).max()
    d, env = case.engine.compress(x, CMP, envelope=True)
    w = O.compress(x, O.profile(CMP, SR))
    ok, worst = C.held(d.to_host(), w)
    assert ok and worst <= 1.0 and C.same_doubles(env.to_host()[0], w.envelope) and np.sum(w.r < 0) > 0
    d.free()
    env.free()


FORMS = dict(plain=dict(), peak=dict(peak=True), stopping=dict(stop_at_silence='own'), pitch=dict(pitch=UP, peak=True),
             everything=dict(pitch=UP, stop_at_silence='own', peak=True, equalizer=EQ))


@pytest.mark.parametrize('form', sorted(FORMS))
def test_a_call_with_the_compressor_is_the_call_then_the_compressor(case, form):
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
    got = case.run(compressor=CMP, **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want)), form
    assert case.engine._compressor is None and case.engine._equalizer is None   # the scope put the handle's settings back
    # the host form: three calls in flight
    peak = kw.pop('peak', False)
    tickets = [case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=peak, compressor=CMP, **kw) for _ in range(3)]
    for t in tickets:
        assert np.array_equal(bits(case.engine.wait_host(t)), bits(want)), form


@pytest.mark.parametrize('stopping', [False, True])
def test_the_loudness_gain_and_the_limiter_run_behind_the_compressor_and_the_equaliser_ahead(case, stopping):
    eng = case.engine
    kw = dict(stop_at_silence=(case.threshold_db, 0)) if stopping else {}
    # everything together: the call with the equaliser alone, the compressor, the loudness normalisation, the limiter
    rows, lens = case.by_hand(peak=False, equalizer=EQ, **kw)
    levelled, gains = eng.loudness_normalize(rows, SR, TARGET[0], TARGET[1], n_samples=lens)
    assert np.any(gains != 1.0)                                          # (a row cut under 400 ms keeps its level: gain 1)
    ceiling = float(np.abs(levelled.to_host()).max()) / 3.0
    limited, stats = eng.limit(levelled, ceiling, L, 4, n_samples=lens)
    want = limited.to_host()
    assert stats['over'].sum() > 0
    settings = dict(compressor=CMP, equalizer=EQ, loudness=TARGET, limiter=(ceiling, MS, 4), **kw)
    got = case.run(peak=False, **settings)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want))
    t = eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=False, **settings)
    assert np.array_equal(bits(eng.wait_host(t)), bits(want))
    # ... and with the limiter alone behind it, on peak-normalised rows
    rows, lens = case.by_hand(peak=True, **kw)
    ceiling = float(np.abs(rows.to_host()).max()) / 3.0
    limited, stats = eng.limit(rows, ceiling, L, 4, n_samples=lens)
    want = limited.to_host()
    got = case.run(peak=True, compressor=CMP, limiter=(ceiling, MS, 4), **kw)['wav'].to_host()
    assert stats['over'].sum() > 0 and np.array_equal(bits(got), bits(want))


def test_an_encoded_output_is_made_of_the_compressed_rows(case):
    rows, _lens = case.by_hand(peak=True)
    want, wst = EO.encode(rows.to_host(), EO.S16, EO.TPDF, SEED)
    codes, n_samples, stats = case.engine.wait_host_encoded(
        case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=True, compressor=CMP, output='pcm16'))
    assert codes.dtype == np.int16 and EC.same_bits(codes, want) and n_samples.tolist() == [want.shape[1]] * case.B
    assert EC.same_records(stats, wst)


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again, or refused: the bits of the handle that never heard of the setting, and no launch in
    stage "compress"; every other stage counts the launches it counted"""
    c, eng = case, case.engine
    eng.set_option('profile', 1)
    stages = ('encoder', 'decoder', 'postnet', 'denorm', 'gl_iter', 'gl_final', 'equalize', 'loudness', 'limiter')
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('compress') == (0.0, 0)
        before = {s: eng.profile_get(s)[1] for s in stages}
        eng.profile_reset()
        on = c.run(compressor=CMP)['wav'].to_host()
        assert eng.profile_get('compress')[1] == 5                       # A, chain A, B, chain B, C
        assert {s: eng.profile_get(s)[1] for s in stages} == before
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('compress') == (0.0, 0) and {s: eng.profile_get(s)[1] for s in stages} == before
    finally:
        eng.set_option('profile', 0)
    assert not np.array_equal(bits(on), bits(c.off))
    # ratio 1 and make-up 0: the setting on, and still the bits of the call as it was
    assert np.array_equal(bits(c.run(compressor=(-20.0, 1.0))['wav'].to_host()), bits(c.off))
    # the profile as numbers is the profile
    assert np.array_equal(bits(c.run(compressor=O.PROFILES[CMP])['wav'].to_host()), bits(on))
    # the handle's setting, read when the call is made
    eng.set_compressor(CMP)
    try:
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
        with pytest.raises(ValueError, match='ratio'):
            eng.set_compressor((-20.0, 0.5))
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))  # refused settings leave the handle's as it was
        assert np.array_equal(bits(c.run(compressor=(-20.0, 1.0))['wav'].to_host()), bits(c.off))
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
    finally:
        eng.set_compressor(None)
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))


def test_synthesize_text_compresses_the_joined_rows():
    """on the texts of tests/test_gpu_long_text.py: every text is the compressor's answer to the text without it (a row's result is
    the bits of its B = 1 call), ahead of the loudness gain where there is one"""
    import test_gpu_long_text as LT
    c = LT.Case()
    try:
        c.hp.magnitude_power, c.engine.sampling_rate = 0.3, SR          # (as that file's loudness test runs them)
        plain = LT.run(c)
        got = LT.run(c, compressor=CMP)
        levelled = LT.run(c, compressor=CMP, loudness=TARGET)
        assert [len(w) for w in got] == [len(w) for w in plain] == [len(w) for w in levelled]
        for g, w in enumerate(plain):
            want = c.engine.compress(w, CMP)
            assert np.array_equal(bits(got[g]), bits(want.to_host())), g
            want, _gains = c.engine.loudness_normalize(want, SR, TARGET[0], TARGET[1])
            assert np.array_equal(bits(levelled[g]), bits(want.to_host())), g
            want.free()
        assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(got, plain))
    finally:
        c.engine.close()
