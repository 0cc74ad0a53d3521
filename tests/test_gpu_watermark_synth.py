"""GPU: the watermark of synthesis (tts_set_watermark).  With the setting on, a call is, bit for bit, the same call made without it
followed by tts_watermark_embed on its rows -- behind the peak normalisation, the equaliser and the compressor, with end-of-speech
stopping (each utterance over the hop (n[b] - 1) samples its row holds), ahead of the loudness gain and of the limiter, in the
device and the host form.  With the setting off the call is the call as it was, and the stage counts no launch.
``synthesize_text`` marks the joined rows.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations) at a power of 0.3 and
8 000 Hz, as tests/test_gpu_loudness_synth.py explains."""
import numpy as np
import pytest

import eos_cases as E
import watermark_cases as C
import watermark_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
TARGET = (-23.0, 1e6)
POWER = 0.3
MS, L = 2.0, 16             # the limiter's look-ahead: 2 ms are 16 samples at 8 kHz
WM = (C.KEY, 0xA5C3)
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
        off = self.run(want_linear=True)              # on a handle whose watermark was never touched
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None

    def args(self):
        c = self.case
        return (self.ids, c['S'], E.REF_DB, E.MAX_DB, POWER, c['n_iter'], c['win'], c['hop'])

    def run(self, peak=False, want_linear=False, **settings):
        return self.engine.synthesize(*self.args(), seed=SEED, peak_normalize=peak, want_linear=want_linear, **settings)

    def by_hand(self, peak=False, **settings):
        """the call without the watermark, then tts_watermark_embed on its rows -> (the device rows, their lengths or None)"""
        out = self.run(peak=peak, **settings)
        lens = self.hop * (out['n_frames'].astype(np.int32) - 1) if 'n_frames' in out else None
        return self.engine.watermark_embed(out['wav'], WM, n_samples=lens), lens


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def test_the_stage_on_a_calls_rows_is_the_oracle(case):
    p = O.params(*WM)
    d = case.engine.watermark_embed(case.off, WM)
    got = d.to_host()
    d.free()
    for b in range(case.B):
        want, marked = O.embed(case.off[b], p)
        assert np.array_equal(bits(got[b]), bits(want)) and marked.sum() > len(want) // 2, b


FORMS = dict(plain=dict(), peak=dict(peak=True), stopping=dict(stop_at_silence='own'),
             everything=dict(stop_at_silence='own', peak=True, equalizer=EQ, compressor=CMP))


@pytest.mark.parametrize('form', sorted(FORMS))
def test_a_call_with_the_watermark_is_the_call_then_the_embedder(case, form):
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
    got = case.run(watermark=WM, **kw)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want)), form
    assert case.engine._watermark is None and case.engine._compressor is None and case.engine._equalizer is None   # the scope put the settings back
    # the host form: three calls in flight
    peak = kw.pop('peak', False)
    tickets = [case.engine.synthesize_host(*case.args(), seed=SEED, peak_normalize=peak, watermark=WM, **kw) for _ in range(3)]
    for t in tickets:
        assert np.array_equal(bits(case.engine.wait_host(t)), bits(want)), form


@pytest.mark.parametrize('stopping', [False, True])
def test_the_loudness_gain_and_the_limiter_run_behind_the_watermark_and_the_compressor_ahead(case, stopping):
    eng = case.engine
    kw = dict(stop_at_silence=(case.threshold_db, 0)) if stopping else {}
    rows, lens = case.by_hand(peak=False, equalizer=EQ, compressor=CMP, **kw)
    levelled, gains = eng.loudness_normalize(rows, SR, TARGET[0], TARGET[1], n_samples=lens)
    assert np.any(gains != 1.0)
    ceiling = float(np.abs(levelled.to_host()).max()) / 3.0
    limited, stats = eng.limit(levelled, ceiling, L, 4, n_samples=lens)
    want = limited.to_host()
    assert stats['over'].sum() > 0 and np.abs(want).max() <= np.float32(ceiling)     # the limiter's ceiling stays exact
    settings = dict(watermark=WM, compressor=CMP, equalizer=EQ, loudness=TARGET, limiter=(ceiling, MS, 4), **kw)
    got = case.run(peak=False, **settings)['wav'].to_host()
    assert np.array_equal(bits(got), bits(want))
    t = eng.synthesize_host(*case.args(), seed=SEED, peak_normalize=False, **settings)
    assert np.array_equal(bits(eng.wait_host(t)), bits(want))


def test_the_setting_off_is_the_call_as_it_was(case):
    """never set, switched on and off again, or refused: the bits of the handle that never heard of the setting, and no launch in
    stage "watermark"; every other stage counts the launches it counted"""
    c, eng = case, case.engine
    eng.set_option('profile', 1)
    stages = ('encoder', 'decoder', 'postnet', 'denorm', 'gl_iter', 'gl_final', 'equalize', 'compress', 'loudness', 'limiter')
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('watermark') == (0.0, 0)
        before = {s: eng.profile_get(s)[1] for s in stages}
        eng.profile_reset()
        on = c.run(watermark=WM)['wav'].to_host()
        assert eng.profile_get('watermark')[1] == 2                      # the blocks' maxima, the marked samples
        assert {s: eng.profile_get(s)[1] for s in stages} == before
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))
        assert eng.profile_get('watermark') == (0.0, 0) and {s: eng.profile_get(s)[1] for s in stages} == before
    finally:
        eng.set_option('profile', 0)
    assert not np.array_equal(bits(on), bits(c.off))
    # no strength: the setting on, and still the bits of the call as it was
    assert np.array_equal(bits(c.run(watermark=WM + (16, 8, 64, 0.0))['wav'].to_host()), bits(c.off))
    # the short forms are the full tuple with the defaults
    assert np.array_equal(bits(c.run(watermark=WM + (16, 8, 64, 0.02))['wav'].to_host()), bits(on))
    # the handle's setting, read when the call is made
    eng.set_watermark(WM)
    try:
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
        with pytest.raises(ValueError, match='chip'):
            eng.set_watermark(WM + (16, 7))
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))  # refused settings leave the handle's as it was
        assert np.array_equal(bits(c.run(watermark=WM + (16, 8, 64, 0.0))['wav'].to_host()), bits(c.off))
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(on))
    finally:
        eng.set_watermark(None)
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off))


def test_synthesize_text_marks_the_joined_rows():
    """on the texts of tests/test_gpu_long_text.py: every text is the embedder's answer to the text without it, so the carrier
    starts at the text's first sample; ahead of the loudness gain where there is one"""
    import test_gpu_long_text as LT
    c = LT.Case()
    try:
        c.hp.magnitude_power, c.engine.sampling_rate = 0.3, SR          # (as that file's loudness test runs them)
        plain = LT.run(c)
        got = LT.run(c, watermark=WM)
        levelled = LT.run(c, watermark=WM, loudness=TARGET)
        assert [len(w) for w in got] == [len(w) for w in plain] == [len(w) for w in levelled]
        for g, w in enumerate(plain):
            want = c.engine.watermark_embed(w, WM)
            assert np.array_equal(bits(got[g]), bits(want.to_host())), g
            want, _gains = c.engine.loudness_normalize(want, SR, TARGET[0], TARGET[1])
            assert np.array_equal(bits(levelled[g]), bits(want.to_host())), g
            want.free()
        assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(got, plain))
    finally:
        c.engine.close()
