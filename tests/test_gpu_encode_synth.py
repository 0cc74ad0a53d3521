"""GPU: the delivery format of synthesis (tts_set_output).  With the setting on, what a ``synthesize_host`` call hands the host is,
bit for bit, the encoder's answer (tests/encode_oracle.py) to the float32 rows of the same call made with the setting off -- behind
the resampler where the rates differ, over the samples each row holds with end-of-speech stopping -- with the call's seed as the
dither's.  The tickets of the two kinds are kept apart, three calls in flight keep their own formats, and with the setting off the
call is the call as it was and the stage counts no launch.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations), the smallest network
the other ``*_synth`` tests use.  A call's outputs are the same bits whatever ran before it, so the float32
rows are taken once."""
import numpy as np
import pytest

import encode_cases as C
import encode_oracle as O
import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
HALF = (22050, 11025)


class Case(object):
    def __init__(self, case):
        self.case = case
        self.engine = pkg().Engine(E.hparams_of(case))
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.hop = case['B'], case['hop']
        # float first, on a handle whose output setting was never touched
        t = self.host(want_linear=True)
        linear, _ = self.engine.wait_host_outputs(t)
        self.w = self.engine.wait_host(t)
        self.N = self.w.shape[1]
        self.threshold_db = E.choose_threshold(linear, case['min_frames'])
        assert self.threshold_db is not None

    def host(self, **kw):
        c = self.case
        return self.engine.synthesize_host(self.ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'], seed=SEED, **kw)


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def _same(got, want_codes, want_records, held):
    codes, n_samples, stats = got
    assert C.same_bits(codes, want_codes)
    assert n_samples.tolist() == list(held)
    assert C.same_records(stats, want_records)


def test_float_first_then_pcm16_on_the_same_handle(case):
    want, wst = O.encode(case.w, O.S16, O.TPDF, SEED)
    assert wst['peak'].min() >= 32767                                        # (peak-normalised rows reach full scale, at +1 or -1)
    got = case.engine.wait_host_encoded(case.host(output='pcm16'))
    assert got[0].dtype == np.int16 and got[0].shape == case.w.shape
    _same(got, want, wst, [case.N] * case.B)
    assert case.engine._output == pkg('_hip').OUTPUT_OFF                                       # the scope put the handle's setting back


@pytest.mark.parametrize('dither', [None, 'tpdf'])
@pytest.mark.parametrize('name', ['pcm16', 'pcm8', 'mulaw', 'alaw'])
def test_every_format_is_the_oracle_on_the_float_rows(case, name, dither):
    fmt = pkg('_hip').FORMATS[name]
    want, wst = O.encode(case.w, fmt, O.TPDF if dither else O.NONE, SEED)
    _same(case.engine.wait_host_encoded(case.host(output=(name, dither, None, None))), want, wst, [case.N] * case.B)


def test_resampling_runs_in_front_of_the_encoder(case):
    eng = case.engine
    r = eng.resample(case.w, 0.5)
    rows = r.to_host()
    r.free()
    N2 = eng.resampled_length(case.N, 0.5)
    assert rows.shape == (case.B, N2)
    want, wst = O.encode(rows, O.S16, O.TPDF, SEED)
    _same(eng.wait_host_encoded(case.host(output=('pcm16', 'tpdf') + HALF)), want, wst, [N2] * case.B)
    # float32 at another rate: the resampler's rows, no records
    codes, n_samples, stats = eng.wait_host_encoded(case.host(output=('float32', None) + HALF))
    assert codes.dtype == np.float32 and C.same_bits(codes, rows) and stats is None and n_samples.tolist() == [N2] * case.B


def test_with_end_of_speech_stopping_the_lengths_are_the_resampled_rows(case):
    eng = case.engine
    stop = (case.threshold_db, 0)
    t = case.host(stop_at_silence=stop)
    frames = eng.wait_host_frames(t)
    w = eng.wait_host(t)
    held = case.hop * (frames.astype(np.int64) - 1)
    assert len(set(held.tolist())) > 1 and held.max() <= case.N
    # at the model's rate
    want, wst = O.encode(w, O.MULAW, O.TPDF, SEED, held)
    t = case.host(stop_at_silence=stop, output='mulaw')
    assert eng.wait_host_frames(t).tolist() == frames.tolist()               # the frames are the call's, as ever
    _same(eng.wait_host_encoded(t), want, wst, held)
    # at half the rate: each row over the samples it holds, into rows of the whole row's resampled length
    N2 = eng.resampled_length(case.N, 0.5)
    r = eng.resample(w, 0.5, n_samples=held.astype(np.int32), N_out=N2)
    rows = r.to_host()
    r.free()
    held2 = [eng.resampled_length(int(n), 0.5) for n in held]
    want, wst = O.encode(rows, O.S16, O.TPDF, SEED, held2)
    _same(eng.wait_host_encoded(case.host(stop_at_silence=stop, output=('pcm16', 'tpdf') + HALF)), want, wst, held2)
    for b, n in enumerate(held2):
        assert not want[b, n:].any()


def test_the_two_kinds_of_ticket_are_kept_apart(case):
    H = pkg('_hip')
    eng = case.engine
    t = case.host(output='alaw')
    with pytest.raises(H.TtsError, match='tts_wait_host_encoded'):
        eng.wait_host(t)
    assert eng.wait_host_encoded(t)[0].dtype == np.uint8                     # ... and the refusal consumed nothing
    t = case.host()
    with pytest.raises(H.TtsError, match='tts_wait_host'):
        eng.wait_host_encoded(t)
    assert C.same_bits(eng.wait_host(t), case.w)


def test_three_calls_in_flight_keep_their_own_formats(case):
    eng = case.engine
    r = eng.resample(case.w, 0.5)
    rows = r.to_host()
    r.free()
    for _round in range(2):
        tickets = [case.host(), case.host(output='pcm16'), case.host(output=('mulaw', None) + HALF)]
        assert C.same_bits(eng.wait_host(tickets[0]), case.w)
        _same(eng.wait_host_encoded(tickets[1]), *O.encode(case.w, O.S16, O.TPDF, SEED), held=[case.N] * case.B)
        _same(eng.wait_host_encoded(tickets[2]), *O.encode(rows, O.MULAW, O.NONE, SEED), held=[rows.shape[1]] * case.B)


def test_the_setting_off_is_the_call_as_it_was(case):
    eng = case.engine
    H = pkg('_hip')
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert C.same_bits(eng.wait_host(case.host()), case.w)
        assert eng.profile_get('encode') == (0.0, 0)
        eng.set_output('pcm16')                                              # the handle's setting, read when the call is made
        want = O.encode(case.w, O.S16, O.TPDF, SEED)
        _same(eng.wait_host_encoded(case.host()), *want, held=[case.N] * case.B)
        assert eng.profile_get('encode')[1] == 2                            # the records and the pass
        for bad in ((5, 0, 0, 0), (1, 2, 0, 0), (1, 0, 22050, 5000), (1, 0, 0, 8000)):
            assert eng.lib.tts_set_output(eng.handle, *bad) == H.TTS_ERR_INVALID, bad
        _same(eng.wait_host_encoded(case.host()), *want, held=[case.N] * case.B)   # refused settings leave the handle's as it was
        # the device form does not read the setting
        c = case.case
        dev = eng.synthesize(case.ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'], seed=SEED)
        assert C.same_bits(dev['wav'].to_host(), case.w)
        eng.set_output(None)
        eng.profile_reset()
        assert C.same_bits(eng.wait_host(case.host()), case.w)
        eng.set_output(('float32', 'tpdf', 22050, 22050))                    # off by another name
        assert C.same_bits(eng.wait_host(case.host()), case.w)
        assert eng.profile_get('encode') == (0.0, 0) and eng.profile_get('resample') == (0.0, 0)
    finally:
        eng.set_option('profile', 0)
        eng.set_output(None)
