"""CPU: what the helpers above the engine (tacotron/inference.py, tacotron/serve.py) share, with no library call.  Every keyword of
``SynthSettings`` through every helper -- taken, and a bad value refused with ValueError before a model, a file or an engine is
touched, or the keyword itself refused with TypeError where the helper cannot honour it -- and the one finishing tail behind
Griffin-Lim (loudness or peak normalisation, limiter, delivery or cut download) through its three callers, on an engine that
records its calls."""
import inspect
import types

import numpy as np
import pytest

from conftest import pkg

# a value of every keyword of the record that is refused with ValueError (and what has to be set beside it for the keyword to be
# looked at): a keyword added to the record fails test_every_keyword_has_a_bad_value until it stands here
BAD = dict(momentum=dict(momentum=2.0), stop_at_silence_db=dict(stop_at_silence_db=float('nan')),
           silence_keep_ms=dict(silence_keep_ms=-1.0, stop_at_silence_db=-40.0), speaking_rate=dict(speaking_rate=9.0),
           pitch=dict(pitch=3.0), phase_init=dict(phase_init='guess'), loudness=dict(loudness=float('nan')),
           check_alignment=dict(check_alignment=True, momentum=2.0),   # (any value switches it on: refused for the momentum beside it)
           pitch_semitones=dict(pitch_semitones=30.0), limiter=dict(limiter=float('nan')), output=dict(output='mp3'),
           marks=dict(marks='syllable'), marks_max_jump=dict(marks_max_jump=0), watermark=dict(watermark='key'),
           compressor=dict(compressor='loud'), equalizer=dict(equalizer='phone'))
IDS = np.ones((2, 5), np.int32)
LIN = np.zeros((2, 40, 1025), np.float32)
NOWHERE = '/nonexistent/weights'


def keywords():
    return [k for k in inspect.signature(pkg('tacotron.inference').SynthSettings.__init__).parameters if k not in ('self', 'hp')]


def helpers(tmp_path):
    """{helper: (a call of it with nothing behind it -- a model that has hyper-parameters only, no weights, no engine --, the
    keywords it does not take)}"""
    I, V = pkg('tacotron.inference'), pkg('tacotron.serve')
    M = types.SimpleNamespace(hparams=pkg('tacotron.params').model_params)
    markup = ('check_alignment',)
    return dict(
        synthesize_batch=(lambda **kw: I.synthesize_batch(M, IDS, **kw), ()),
        synthesize_stream=(lambda **kw: next(I.synthesize_stream(M, [IDS], **kw)), ()),
        inference_stream=(lambda **kw: next(I.inference_stream(M, [IDS], **kw)), tuple(k for k in keywords() if k not in ('momentum', 'phase_init'))),
        synthesize_sentences=(lambda **kw: I.synthesize_sentences(['x'], NOWHERE, out_dir='/nonexistent', **kw), ()),
        synthesize_marked=(lambda **kw: I.synthesize_marked(M, ['x'], None, **kw), markup),
        synthesize_marked_sentences=(lambda **kw: I.synthesize_marked_sentences(['x'], NOWHERE, out_dir='/nonexistent', **kw), markup),
        synthesize_text=(lambda **kw: I.synthesize_text(M, ['x'], None, **kw), ()),
        synthesize_texts=(lambda **kw: I.synthesize_texts(['x'], NOWHERE, out_dir=str(tmp_path), **kw), ()),   # (it looks at out_dir first)
        serve=(lambda **kw: next(V.serve(iter([['x']]), NOWHERE, **kw)), ()),
        post_process_spectrograms=(lambda **kw: V.post_process_spectrograms(LIN, None, **kw), ('check_alignment', 'output', 'marks', 'marks_max_jump')))


def test_every_keyword_has_a_bad_value():
    assert sorted(BAD) == sorted(keywords())
    assert all(k in BAD[k] for k in BAD)


def test_every_helper_takes_every_keyword_or_refuses_it(tmp_path):
    table = helpers(tmp_path)
    I, V = pkg('tacotron.inference'), pkg('tacotron.serve')
    public = {n for m in (I, V) for n, f in vars(m).items() if callable(f) and hasattr(f, 'parts')}
    assert sorted(public) == sorted(table)                       # every helper that takes the settings is looked at here
    for name, (call, refused) in sorted(table.items()):
        taken = inspect.signature(getattr(I, name, None) or getattr(V, name)).parameters
        for keyword in keywords():
            if keyword in refused:
                assert keyword not in taken, (name, keyword)
                with pytest.raises(TypeError) as e:
                    call(**{keyword: BAD[keyword][keyword]})
                assert "unexpected keyword argument '{}'".format(keyword) in str(e.value), (name, keyword)
            else:
                assert keyword in taken, (name, keyword)
                with pytest.raises(ValueError):
                    call(**BAD[keyword])
        with pytest.raises(TypeError):
            call(tempo=1.0)
    for name in ('synthesize_marked', 'synthesize_marked_sentences'):   # a pitch is taken, and only 0 is honoured
        for shift in (dict(pitch=0.5), dict(pitch_semitones=2.0)):
            with pytest.raises(ValueError) as e:
                table[name][0](**shift)
            assert str(e.value).startswith('synthesize_marked: a pitch other than 0 is not supported with markup'), name


# ---------------------------------------------------------------------------------------------- the finishing tail
HOP, SR = 275, 22050


class Dev(object):
    """a device array: a host array with ``to_host`` and ``free``"""

    def __init__(self, a):
        self.a = np.asarray(a)
        self.shape, self.dtype = self.a.shape, self.a.dtype

    def to_host(self):
        return self.a.reshape(self.shape)

    def free(self):
        pass


class TailEngine(object):
    """the stages the three callers compose, answered with zeros of the right shapes; ``calls``: ``(name, n_samples)`` of every one"""
    sampling_rate = SR

    def __init__(self, n_frames=(30, 12)):
        self.calls, self.n_frames, self.kept = [], n_frames, {}

    def note(self, name, n_samples=None, **kept):
        self.calls.append((name, None if n_samples is None else np.asarray(n_samples).tolist()))
        self.kept[name] = kept

    def names(self, behind=None):
        names = [n for n, _ in self.calls]
        return names if behind is None else names[len(names) - names[::-1].index(behind):]

    # the network and what stands in front of Griffin-Lim
    def encoder_forward(self, ids):
        self.note('encoder_forward')
        self.B, self.Ts = ids.shape
        return Dev(np.zeros((self.B, self.Ts, 256), np.float32))

    def decoder_forward(self, memory, S):
        self.note('decoder_forward')
        self.S = S
        return Dev(np.zeros((self.B, S, 400), np.float32)), Dev(np.zeros((S, self.B, self.Ts), np.float32))

    def token_times(self, alignments, n_sent=None, max_jump=4, to_host=True):
        self.note('token_times')
        start = np.tile(np.minimum(np.arange(self.Ts + 1), self.S).astype(np.int32), (self.B, 1))   # one step per token, while they last
        return Dev(start), Dev(np.zeros(self.B, pkg('_hip').TOKEN_TIMES_RECORD))

    def postnet_forward(self, mel):
        self.note('postnet_forward')
        return Dev(np.zeros(mel.shape[:2] + (1025,), np.float32))

    def speech_threshold(self, db, ref_db, max_db):
        self.note('speech_threshold')
        return 0.5

    def speech_frames(self, spec, threshold, keep_frames=0, min_frames=1):
        self.note('speech_frames')
        return Dev(np.array(self.n_frames, np.int32)), Dev(np.zeros(len(self.n_frames), np.int32))

    def speech_interval(self, linear, threshold):
        self.note('speech_interval')
        return Dev(np.zeros(linear.shape[0], np.int32)), Dev(np.zeros(linear.shape[0], np.int32))

    def denorm_power(self, spec, ref_db, max_db, power):
        self.note('denorm_power')
        return Dev(np.zeros((spec.shape[0], 1025, spec.shape[1]), np.float32))

    def warp_magnitudes(self, mag, segments, n_frames):
        self.note('warp_magnitudes')
        n_out = np.zeros(mag.shape[0], np.int64)
        for row, _first, frames, pause, step, _gain in segments:
            n_out[row] += pause if frames == 0 else pkg('tacotron.prosody').warp_count(frames, step)
        return Dev(np.zeros((mag.shape[0], 1025, int(n_out.max())), np.float32)), n_out

    def griffin_lim(self, mag, n_iter, win_len, hop, n_fft, n_frames=None, **keywords):
        self.note('griffin_lim')
        return Dev(np.zeros((mag.shape[0], hop * (mag.shape[2] - 1)), np.float32)), None

    def synthesize(self, ids, S, *args, **keywords):
        self.note('synthesize', **keywords)
        B = len(ids)
        return dict(wav=Dev(np.zeros((B, HOP * (5 * S - 1)), np.float32)), linear=Dev(np.zeros((B, 5 * S, 1025), np.float32)),
                    n_frames=np.array(self.n_frames[:B], np.int32))

    def join(self, wav, pieces, groups, fade):
        self.note('join')
        n_out = np.zeros(int(groups.max()) + 1, np.int64)
        for (_row, _first, count, gap), g in zip(pieces, groups):
            n_out[g] += count + gap
        self.n_out = n_out
        return Dev(np.zeros((len(n_out), int(n_out.max())), np.float32)), n_out

    # the tail
    def loudness_normalize(self, rows, sampling_rate, target, max_peak, n_samples=None):
        self.note('loudness_normalize', n_samples)

    def peak_normalize(self, rows):
        self.note('peak_normalize')

    def limit(self, rows, ceiling, lookahead=0, oversample=4, n_samples=None):
        self.note('limit', n_samples, lookahead=lookahead)

    def resample(self, rows, ratio, n_samples=None, N_out=None):
        self.note('resample', n_samples)
        return Dev(np.zeros((rows.shape[0], N_out), np.float32))

    def encode(self, rows, fmt, dither=None, seed=0, n_samples=None):
        self.note('encode', n_samples, seed=seed)
        return Dev(np.zeros(rows.shape, np.int16)), None

    def download_rows(self, rows, lengths):
        self.note('download_rows', lengths)
        return [rows.to_host()[g, :int(n)] for g, n in enumerate(lengths)]

    def to_device(self, batch):
        self.note('to_device')
        return Dev(batch)


def dataset():
    P = pkg('tacotron.params')
    return pkg('datasets.lj_speech').LJSpeechDatasetHelper('/nonexistent', dict(P.dataset_params.vocabulary_dict), False)


def model_of(eng, n_steps=4):
    return types.SimpleNamespace(hparams=pkg('tacotron.params').model_params, n_steps=lambda: n_steps, engine=eng)


LOUD = dict(loudness=-20.0, limiter=0.5)
TOO_FAR = (0.5, 50.0, 4)                                         # 50 ms are 1102 samples at 22 050 Hz, and 1024 is the most


def test_the_tail_of_synthesize_marked():
    I = pkg('tacotron.inference')
    marked = ['one two', 'one <break time="300ms"/>two']

    def run(**kw):
        eng = TailEngine()
        wavs, plan = I.synthesize_marked(model_of(eng), marked, dataset(), want_plan=True, **kw)
        held = [HOP * (n - 1) for n in plan['n_out']]
        assert held[1] - held[0] == HOP * 24                     # (the break: 24 frames)
        return eng, held, [len(w) for w in wavs]

    eng, held, lengths = run(peak_normalize=True, output=('pcm16', 'tpdf', 11025), seed=7, **LOUD)
    half = [pkg('_hip').resampled_length(n, 0.5) for n in held]
    assert eng.calls[eng.names().index('griffin_lim') + 1:] == [('loudness_normalize', held), ('limit', held), ('resample', held),
                                                               ('encode', half)]
    assert lengths == half
    assert eng.kept['limit'] == dict(lookahead=110) and eng.kept['encode'] == dict(seed=7)
    eng, held, lengths = run(peak_normalize=True, limiter=0.5)   # a peak normalisation only where there is no loudness
    assert eng.calls[eng.names().index('griffin_lim') + 1:] == [('peak_normalize', None), ('limit', held), ('download_rows', held)]
    assert lengths == held
    eng, held, lengths = run()
    assert eng.calls[eng.names().index('griffin_lim') + 1:] == [('download_rows', held)] and lengths == held
    eng = TailEngine()
    with pytest.raises(ValueError) as e:
        I.synthesize_marked(model_of(eng), marked, dataset(), limiter=TOO_FAR)
    assert str(e.value) == 'synthesize_marked: a look-ahead of 50.0 ms is 1102 samples at 22050 Hz, more than 1024' and eng.calls == []


def test_the_tail_of_synthesize_text():
    I = pkg('tacotron.inference')
    texts = ['One. Two.', 'Three.']
    eng = TailEngine(n_frames=(12, 9, 7))
    wavs = I.synthesize_text(model_of(eng), texts, dataset(), output='pcm16', peak_normalize=I.SynthSettings(None, **LOUD).file_norm()[0], **LOUD)
    held = eng.n_out.tolist()
    assert len(held) == 2 and held[0] > held[1] > 0 and [len(w) for w in wavs] == held
    assert eng.kept['synthesize']['loudness'] is None and eng.kept['synthesize']['limiter'] is None   # both run on the joined rows
    assert eng.calls[eng.names().index('join') + 1:] == [('loudness_normalize', held), ('limit', held), ('download_rows', held),
                                                        ('to_device', None), ('encode', held)]
    assert eng.kept['limit'] == dict(lookahead=110)
    eng = TailEngine(n_frames=(12, 9, 7))                        # the whole texts are peak-normalised ahead of the encoder, not the rows
    I.synthesize_text(model_of(eng), texts, dataset(), output='pcm16', peak_normalize=True)
    assert eng.names('join') == ['download_rows', 'to_device', 'peak_normalize', 'encode']
    eng = TailEngine(n_frames=(12, 9, 7))
    with pytest.raises(ValueError) as e:
        I.synthesize_text(model_of(eng), texts, dataset(), limiter=TOO_FAR)
    assert str(e.value) == 'synthesize_text: a look-ahead of 50.0 ms is 1102 samples at 22050 Hz, more than 1024' and eng.calls == []


def test_the_tail_of_post_process_spectrograms():
    V = pkg('tacotron.serve')
    eng = TailEngine()
    held = [HOP * (n - 1) for n in eng.n_frames]
    wavs = V.post_process_spectrograms(LIN, eng, stop_at_silence_db=-40.0, **LOUD)
    assert eng.calls[eng.names().index('griffin_lim') + 1:] == [('loudness_normalize', held), ('limit', held), ('download_rows', held)]
    assert [len(w) for w in wavs] == held and eng.kept['limit'] == dict(lookahead=110)
    eng = TailEngine()
    wavs = V.post_process_spectrograms(LIN, eng, **LOUD)         # without stopping every row holds all its samples
    assert eng.calls[eng.names().index('griffin_lim') + 1:] == [('loudness_normalize', None), ('limit', None)]
    assert [len(w) for w in wavs] == [HOP * 39] * 2 and 'peak_normalize' not in eng.names()
    eng = TailEngine()
    with pytest.raises(ValueError) as e:
        V.post_process_spectrograms(LIN, eng, limiter=TOO_FAR)
    assert str(e.value) == 'post_process_spectrograms: a look-ahead of 50.0 ms is 1102 samples at 22050 Hz, more than 1024' and eng.calls == []
