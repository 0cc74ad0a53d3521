"""The per-call synthesis settings of the binding (_hip.py), pinned with no library and no GPU: which ``tts_set_*`` /
``tts_set_option`` calls surround a ``tts_synthesize*`` / ``tts_griffin_lim*`` call, in which order, and what the seven mirror
attributes hold afterwards.  The library is a stand-in that records every call; the expected sequences are literals, recorded
from the binding as it stood when every setting had a scope object of its own."""
import numpy as np
import pytest

from conftest import pkg
from host_checks import no_device_engine

MIRRORS = ('_gl_momentum', '_end_of_speech', '_speaking_rate', '_pitch', '_gl_init', '_loudness', '_alignment_stats')
INITIAL = (0, (False, 0.0, 0), 1.0, 0.0, 0, None, (False, 0))
TRACED = ('tts_set_', 'tts_synthesize', 'tts_griffin_lim')
SYN = (2, 6.02, 99.89, 1.3, 2, 1102, 275)   # n_steps, ref_db, max_db, power, n_iter, win_length, hop_length
ALL = dict(momentum=0.5, stop_at_silence=(-30.0, 2), speaking_rate=1.25, pitch=0.25, phase_init='estimate', loudness=-20.0,
           alignment_stats=(True, 3))

# (the setter call that applies each keyword of ALL, the one that puts the handle's initial value back)
SET = dict(momentum=(('tts_set_option', (b'gl_momentum', 500)), ('tts_set_option', (b'gl_momentum', 0))),
           stop_at_silence=(('tts_set_end_of_speech', (1, -30.0, 2)), ('tts_set_end_of_speech', (0, 0.0, 0))),
           speaking_rate=(('tts_set_speaking_rate', (1.25,)), ('tts_set_speaking_rate', (1.0,))),
           pitch=(('tts_set_pitch', (0.25,)), ('tts_set_pitch', (0.0,))),
           phase_init=(('tts_set_option', (b'gl_init', 1)), ('tts_set_option', (b'gl_init', 0))),
           loudness=(('tts_set_loudness', (1, -20.0, 1.0, 22050)), ('tts_set_loudness', (0, 0.0, 1.0, 0))),
           alignment_stats=(('tts_set_alignment_stats', (1, 3)), ('tts_set_alignment_stats', (0, 0))))
ORDER = ('momentum', 'stop_at_silence', 'speaking_rate', 'pitch', 'phase_init', 'loudness', 'alignment_stats')
CALLS = {'synthesize': ('tts_synthesize', (2, 5)), 'synthesize_host': ('tts_synthesize_host', (2, 5))}
GL = ('tts_griffin_lim', (0, 1, 12, 2, 1102, 275, 2048))
GL_RAGGED = ('tts_griffin_lim_ragged', (0, 1, 12, 2, 1102, 275, 2048))


class RecordingLibrary(object):
    """every ``tts_*`` attribute is a function that appends ``(name, the scalar arguments)`` to ``calls`` and returns TTS_OK
    -- or what ``refuse`` holds for the name; ``tts_last_error`` returns b''"""

    def __init__(self):
        self.calls, self.refuse = [], {}

    def __getattr__(self, name):
        if not name.startswith('tts_'):
            raise AttributeError(name)

        def call(*args):
            if name == 'tts_last_error':
                return b''
            self.calls.append((name, tuple(a for a in args if isinstance(a, (int, float, bytes)))))
            return self.refuse.get(name, 0)
        return call

    def trace(self):
        # (the host form's first scalar is the address of its ids)
        return [(n, a[-2:] if n == 'tts_synthesize_host' else a) for n, a in self.calls if n.startswith(TRACED)]


@pytest.fixture
def eng():
    H = pkg('_hip')
    e = no_device_engine()
    e.lib = RecordingLibrary()
    e.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    e._staging, e._host_shapes, e._host_out_shapes = {}, {}, {}
    assert mirrors(e) == INITIAL
    return e


def mirrors(e):
    return tuple(getattr(e, a) for a in MIRRORS)


def run(e, method, **keywords):
    return getattr(e, method)(np.ones((2, 5), np.int32), *SYN, **keywords)


def test_the_one_table_has_every_keyword_in_the_order_it_is_applied_in():
    H = pkg('_hip')
    assert [row.keyword for row in H.SETTINGS] == list(ORDER) + ['limiter', 'output', 'token_times', 'watermark', 'compressor', 'equalizer']
    assert len({row.mirror for row in H.SETTINGS}) == 13 and [row.keyword for row in H.SETTINGS if row.host_only] == ['output']
    assert tuple(row.mirror for row in H.SETTINGS[:7]) == MIRRORS and tuple(row.initial for row in H.SETTINGS[:7]) == INITIAL


@pytest.mark.parametrize('method', sorted(CALLS))
def test_no_keyword_no_setter(eng, method):
    run(eng, method)
    assert eng.lib.trace() == [CALLS[method]]
    assert mirrors(eng) == INITIAL


@pytest.mark.parametrize('method', sorted(CALLS))
@pytest.mark.parametrize('keyword', ORDER)
def test_each_keyword_alone_is_set_and_put_back(eng, method, keyword):
    run(eng, method, **{keyword: ALL[keyword]})
    assert eng.lib.trace() == [SET[keyword][0], CALLS[method], SET[keyword][1]]
    assert mirrors(eng) == INITIAL


@pytest.mark.parametrize('method', sorted(CALLS))
def test_all_seven_are_set_in_order_and_put_back_in_reverse(eng, method):
    run(eng, method, **ALL)
    assert eng.lib.trace() == [SET[k][0] for k in ORDER] + [CALLS[method]] + [SET[k][1] for k in reversed(ORDER)]
    assert mirrors(eng) == INITIAL


@pytest.mark.parametrize('method', sorted(CALLS))
def test_a_keyword_equal_to_the_handles_value_sets_nothing(eng, method):
    eng.set_speaking_rate(1.25)
    del eng.lib.calls[:]
    run(eng, method, speaking_rate=1.25)
    assert eng.lib.trace() == [CALLS[method]]
    assert mirrors(eng) == INITIAL[:2] + (1.25,) + INITIAL[3:]


def test_a_call_made_with_stopping_reports_its_frames(eng):
    assert 'n_frames' not in run(eng, 'synthesize')
    assert 'n_frames' in run(eng, 'synthesize', stop_at_silence=(-30.0, 2))
    eng.set_end_of_speech(True, -30.0, 2)
    assert 'n_frames' in run(eng, 'synthesize')


def test_the_host_call_sizes_its_waveforms_by_the_calls_rate(eng):
    t = run(eng, 'synthesize_host', speaking_rate=1.25)
    assert eng._host_shapes[t] == (2, 275 * 7)   # ceil(10 / 1.25) = 8 frames
    eng.set_speaking_rate(2.0)
    t = run(eng, 'synthesize_host')
    assert eng._host_shapes[t] == (2, 275 * 4)


@pytest.mark.parametrize('method', sorted(CALLS))
def test_a_refused_call_is_followed_by_every_put_back(eng, method):
    H = pkg('_hip')
    eng.lib.refuse[CALLS[method][0]] = H.TTS_ERR_INVALID
    with pytest.raises(H.TtsError):
        run(eng, method, **ALL)
    assert eng.lib.trace() == [SET[k][0] for k in ORDER] + [CALLS[method]] + [SET[k][1] for k in reversed(ORDER)]
    assert mirrors(eng) == INITIAL


@pytest.mark.parametrize('method', sorted(CALLS))
def test_a_refused_setter_puts_back_what_was_entered_and_makes_no_call(eng, method):
    H = pkg('_hip')
    eng.lib.refuse['tts_set_pitch'] = H.TTS_ERR_INVALID
    with pytest.raises(H.TtsError):
        run(eng, method, **ALL)
    entered = ORDER[:3]
    assert eng.lib.trace() == [SET[k][0] for k in entered] + [SET['pitch'][0]] + [SET[k][1] for k in reversed(entered)]
    assert mirrors(eng) == INITIAL


@pytest.mark.parametrize('n_frames, call', [(None, GL), ([12], GL_RAGGED)])
def test_griffin_lim_sets_its_two(eng, n_frames, call):
    H = pkg('_hip')
    mag = np.ones((1, 1025, 12), np.float32)
    eng.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=n_frames)
    assert eng.lib.trace() == [call]
    del eng.lib.calls[:]
    eng.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=n_frames, momentum=0.5, phase_init='estimate')
    assert eng.lib.trace() == [SET['momentum'][0], SET['phase_init'][0], call, SET['phase_init'][1], SET['momentum'][1]]
    del eng.lib.calls[:]
    eng.lib.refuse[call[0]] = H.TTS_ERR_INVALID
    with pytest.raises(H.TtsError):
        eng.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=n_frames, momentum=0.5, phase_init='estimate')
    assert eng.lib.trace() == [SET['momentum'][0], SET['phase_init'][0], call, SET['phase_init'][1], SET['momentum'][1]]
    del eng.lib.calls[:]
    eng.lib.refuse = {'tts_set_option': H.TTS_ERR_INVALID}
    with pytest.raises(H.TtsError):
        eng.griffin_lim(mag, 2, 1102, 275, 2048, n_frames=n_frames, momentum=0.5, phase_init='estimate')
    assert eng.lib.trace() == [SET['momentum'][0]]
    assert mirrors(eng) == INITIAL


def test_set_option_keeps_its_two_mirrors(eng):
    eng.set_option('gl_momentum', 250)
    assert mirrors(eng) == (250,) + INITIAL[1:]
    eng.set_option('gl_init', 1)
    assert mirrors(eng) == (250,) + INITIAL[1:4] + (1,) + INITIAL[5:]
    eng.set_option('pd_ws', 1)
    assert mirrors(eng) == (250,) + INITIAL[1:4] + (1,) + INITIAL[5:]
    assert eng.lib.trace() == [('tts_set_option', (b'gl_momentum', 250)), ('tts_set_option', (b'gl_init', 1)), ('tts_set_option', (b'pd_ws', 1))]


def test_a_bad_value_is_refused_before_a_handle_is_touched(eng):
    for keywords in (dict(ALL, alignment_stats=3), dict(ALL, momentum=1.0), dict(ALL, pitch=float('nan'))):
        for method in sorted(CALLS):
            with pytest.raises(ValueError):
                run(eng, method, **keywords)
    assert eng.lib.calls == []
    assert mirrors(eng) == INITIAL


class KeywordEngine(object):
    """an engine that keeps the setting keywords of every synthesis call made on it and answers with zeros"""

    def __init__(self):
        self.seen = []

    def _call(self, ids, keywords):
        self.seen.append({k: keywords[k] for k in ORDER})
        return np.zeros((len(ids), 275 * 9), np.float32)

    def synthesize(self, ids, *args, **keywords):
        wav = self._call(ids, keywords)
        return dict(wav=type('Dev', (), {'to_host': lambda self: wav})(), n_frames=np.full(len(ids), 4, np.int32))

    def synthesize_host(self, ids, *args, **keywords):
        self._call(ids, keywords)
        return len(self.seen)

    def wait_host(self, ticket, copy=True):
        return np.zeros((2, 275 * 9), np.float32)

    def wait_host_frames(self, ticket):
        return np.full(2, 4, np.int32)

    def synth_alignment_stats(self, B):
        return np.ones(B, pkg('_hip').ALIGNMENT_RECORD)

    def wait_host_alignment_stats(self, ticket):
        return self.synth_alignment_stats(2)


LAYER_CASES = [
    (dict(), dict(momentum=0.0, stop_at_silence=None, speaking_rate=1.0, pitch=0.0, phase_init='random', loudness=None, alignment_stats=None)),
    (dict(speaking_rate=None, pitch=None, phase_init=None),
     dict(momentum=0.0, stop_at_silence=None, speaking_rate=1.0, pitch=0.0, phase_init=None, loudness=None, alignment_stats=None)),
    (dict(momentum=0.5, stop_at_silence_db=-40.0, silence_keep_ms=30.0, speaking_rate=1.25, pitch=0.25, phase_init='estimate', loudness=-20,
          check_alignment=True),
     dict(momentum=0.5, stop_at_silence=(-40.0, 3), speaking_rate=1.25, pitch=0.25, phase_init='estimate', loudness=(-20.0, 1.0),
          alignment_stats=(True, 0))),
    (dict(stop_at_silence_db=-35, loudness=(-16.0, 0.5), check_alignment=1),
     dict(momentum=0.0, stop_at_silence=(-35.0, 9), speaking_rate=1.0, pitch=0.0, phase_init='random', loudness=(-16.0, 0.5),
          alignment_stats=(True, 0))),
]


@pytest.mark.parametrize('given, handed', LAYER_CASES)
def test_what_the_layer_above_hands_the_engine(given, handed):
    """synthesize_batch and synthesize_stream: this layer's keywords as the engine's (hops of 275 samples: 30 ms are 3 frames,
    the default 100 ms are 9; the pad id is 0)"""
    import types
    I = pkg('tacotron.inference')
    ids = np.ones((2, 5), np.int32)
    for call in (lambda m: I.synthesize_batch(m, ids, **given), lambda m: list(I.synthesize_stream(m, [ids], **given))):
        model = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params, n_steps=lambda: 2, engine=KeywordEngine())
        call(model)
        assert model.engine.seen == [handed]
