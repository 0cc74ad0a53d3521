"""GPU: the seven per-call synthesis settings together (_hip.SETTINGS).  One call made with every keyword at once is, bit for
bit, the call made with no keyword after the same values were put on the handle by its set_* calls and options; the host form
gives the device form's bits; afterwards the handle is as it was, also when the library refused the call inside the block.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations), the fixture network
at a power of 0.3 with the loudness measured at 8 000 Hz, as test_gpu_loudness_synth.py explains; the rate and the pitch are the
pair test_gpu_pitch.py runs together."""
import numpy as np
import pytest

import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
POWER = 0.3
PAD_ID = 0                  # (eos_cases.ids_of pads its short sentence with 0)
MIRRORS = ('_gl_momentum', '_end_of_speech', '_speaking_rate', '_pitch', '_gl_init', '_loudness', '_alignment_stats')
INITIAL = (0, (False, 0.0, 0), 1.0, 0.0, 0, None, (False, 0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(object):
    def __init__(self, case):
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.sampling_rate = SR
        self.engine.load_weights(E.weights_of(case))
        self.B = case['B']
        self.args = (E.ids_of(case), case['S'], E.REF_DB, E.MAX_DB, POWER, case['n_iter'], case['win'], case['hop'])
        plain = self.run(want_linear=True)
        self.plain = plain['wav'].to_host()
        threshold_db = E.choose_threshold(plain['linear'].to_host(), case['min_frames'])
        assert threshold_db is not None
        self.keywords = dict(momentum=0.5, stop_at_silence=(float(threshold_db), 0), speaking_rate=1.2, pitch=4.0 / 12.0, phase_init='estimate',
                             loudness=(-23.0, 1e6), alignment_stats=(True, PAD_ID))

    def run(self, **keywords):
        return self.engine.synthesize(*self.args, seed=SEED, peak_normalize=False, **keywords)

    def mirrors(self):
        return tuple(getattr(self.engine, a) for a in MIRRORS)

    def result(self, **keywords):
        """(waveforms, reported lengths, alignment records) of a device call"""
        out = self.run(**keywords)
        return out['wav'].to_host(), self.engine.synth_frames(self.B), self.engine.synth_alignment_stats(self.B)


def same(got, want):
    return (np.array_equal(bits(got[0]), bits(want[0])) and got[0].shape == want[0].shape and np.array_equal(got[1], want[1]) and
            got[2].tobytes() == want[2].tobytes())


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


@pytest.fixture(scope='module')
def by_keywords(case):
    """the call made with all seven keywords at once; the handle afterwards"""
    got = case.result(**case.keywords)
    assert case.mirrors() == INITIAL
    assert len(set(got[1].tolist())) > 1 and got[0].shape != case.plain.shape and got[2].shape == (case.B,) and (got[2]['n_sent'] > 0).all()
    return got


def test_the_keywords_are_the_handles_settings(case, by_keywords):
    eng, k = case.engine, case.keywords
    eng.set_option('gl_momentum', 500)
    eng.set_end_of_speech(True, *k['stop_at_silence'])
    eng.set_speaking_rate(k['speaking_rate'])
    eng.set_pitch(k['pitch'])
    eng.set_option('gl_init', 1)
    eng.set_loudness(k['loudness'])
    eng.set_alignment_stats(*k['alignment_stats'])
    try:
        assert case.mirrors() == (500, (True,) + k['stop_at_silence'], k['speaking_rate'], k['pitch'], 1, k['loudness'], k['alignment_stats'])
        out = case.run()
        assert np.array_equal(out['n_frames'], by_keywords[1])
        assert same((out['wav'].to_host(), eng.synth_frames(case.B), eng.synth_alignment_stats(case.B)), by_keywords)
    finally:
        eng.set_alignment_stats(False)
        eng.set_loudness(None)
        eng.set_option('gl_init', 0)
        eng.set_pitch(0.0)
        eng.set_speaking_rate(1.0)
        eng.set_end_of_speech(False)
        eng.set_option('gl_momentum', 0)
    assert case.mirrors() == INITIAL


def test_the_host_form_is_the_device_form(case, by_keywords):
    eng = case.engine
    t = eng.synthesize_host(*case.args, seed=SEED, peak_normalize=False, **case.keywords)
    assert case.mirrors() == INITIAL
    assert same((eng.wait_host(t), eng.wait_host_frames(t), eng.wait_host_alignment_stats(t)), by_keywords)


def test_the_handle_is_left_as_it_was(case, by_keywords):
    assert case.mirrors() == INITIAL
    assert np.array_equal(bits(case.run()['wav'].to_host()), bits(case.plain))
    t = case.engine.synthesize_host(*case.args, seed=SEED, peak_normalize=False)
    assert np.array_equal(bits(case.engine.wait_host(t)), bits(case.plain))


def test_a_call_refused_inside_the_block_leaves_the_handle_as_it_was(case, by_keywords):
    """a rate and a pitch whose product leaves [0.25, 4]: the binding hands them on (no init_phase), the library refuses the call"""
    H = pkg('_hip')
    with pytest.raises(H.TtsError) as e:
        case.run(**dict(case.keywords, speaking_rate=2.5, pitch=-1.0))
    assert e.value.code == H.TTS_ERR_INVALID and 'pitch' in str(e.value)
    assert case.mirrors() == INITIAL
    assert np.array_equal(bits(case.run()['wav'].to_host()), bits(case.plain))
