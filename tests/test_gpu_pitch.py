"""GPU: the pitch of synthesis (tts_set_pitch) and Engine.pitch_shift.  A shifted call is, bit for bit, the stage calls chained by
hand on the call's own magnitudes: tts_stretch_rows by s * rho (rho = 2 ** -octaves, s the speaking rate), Griffin-Lim from the
same seed without normalisation, tts_resample by rho into the rows of the call without pitch, tts_peak_normalize -- and it
changes no shape and no reported length (reference audio/effects.py:9-43: time_stretch at 2 ** -octaves, then librosa's
resampler and fix_length).  Pitch 0 is the call as it was.

Shapes: the streaming end-to-end case of eos_cases.py (B = 3, T = 40 frames of 275 samples, 3 iterations)."""
import numpy as np
import pytest

import eos_cases as E
import resample_oracle as R
import stretch_oracle as S
from conftest import pkg

pytestmark = pytest.mark.gpu

UP, DOWN = 4.0 / 12.0, -4.0 / 12.0
SEED = 9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case(object):
    def __init__(self, case):
        self.case = case
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.T = case['B'], case['S'] * self.hp.reduction
        self.hop, self.F = case['hop'], 1 + case['n_fft'] // 2
        self.FP = (self.F + 31) // 32 * 32            # the padded rows of the call's magnitudes
        off = self.run(want=True)                     # on a handle whose pitch was never touched
        self.off = {k: off[k].to_host() for k in ('wav', 'mel', 'linear', 'alignments')}
        self.threshold_db = E.choose_threshold(self.off['linear'], case['min_frames'])
        assert self.threshold_db is not None
        self.stop = (self.threshold_db, 0)
        self.detected = self.run(stop=self.stop)['n_frames']
        assert len(set(self.detected.tolist())) == self.B

    def run(self, pitch=None, rate=None, stop=None, peak=False, want=False, momentum=None, seed=SEED):
        c = self.case
        return self.engine.synthesize(self.ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'], seed=seed,
                                      peak_normalize=peak, want_mel=want, want_linear=want, want_alignments=want, momentum=momentum,
                                      stop_at_silence=stop, speaking_rate=rate, pitch=pitch)

    def lengths(self, rate, T_r):
        """min(T_r, max(min_frames, stretched_frames(n, rate))) of the detected lengths; rate 1: the lengths themselves"""
        if rate == 1.0:
            return self.detected.copy()
        return S.stretched_lengths(self.detected, rate, T_r, self.case['min_frames'])

    def chain(self, octaves, s, stop, peak):
        """the stage calls by hand, on the magnitudes the last call left in the handle's workspace"""
        c, eng = self.case, self.engine
        rho = float(np.exp2(-np.float64(octaves)))
        eff = s * rho
        Tg = S.stretched_frames(self.T, eff)
        Tw = self.T if s == 1.0 else S.stretched_frames(self.T, s)
        magi = eng.debug_workspace('gl.mag', (self.B, self.T, self.FP))
        det = self.detected if stop else None
        rows = eng.stretch_rows(magi[:, :, :self.F], eff, n_frames=det, T_out=Tg, row_stride=self.FP)
        mag = np.ascontiguousarray(rows.to_host()[:, :, :self.F].transpose(0, 2, 1))
        n_gl = self.lengths(eff, Tg) if stop else None
        n_s = self.lengths(s, Tw) if stop else None
        wav, _ = eng.griffin_lim(mag, c['n_iter'], c['win'], c['hop'], c['n_fft'], seed=SEED, want_mse=False, n_frames=n_gl)
        assert wav.shape == (self.B, self.hop * (Tg - 1))
        N_out = self.hop * (Tw - 1)
        out = eng.resample(wav, rho, n_samples=None if n_gl is None else self.hop * (n_gl - 1), N_out=N_out).to_host()
        keep = []
        for b in range(self.B):
            n_in = self.hop * ((int(n_gl[b]) if stop else Tg) - 1)
            k = min(R.resampled_valid(n_in, rho), self.hop * (int(n_s[b]) - 1) if stop else N_out)
            out[b, k:] = 0.0           # (the row ends where the un-shifted call's does)
            keep.append(k)
        if peak:
            out = eng.peak_normalize(eng.to_device(out)).to_host()
        return out, n_s, keep


@pytest.fixture(scope='module')
def case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


def test_pitch_zero_is_the_call_as_it_was(case):
    """never set, set to 0, or set to something else and back: the bits of the handle that never heard of the setting, and no
    launch in stage "resample" """
    c, eng = case, case.engine
    H = pkg('_hip')
    want = c.off['wav']
    assert np.array_equal(bits(c.run(pitch=0.0)['wav'].to_host()), bits(want))
    c.run(pitch=UP)
    assert eng._pitch == 0.0            # the scope put the handle's setting back
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run()['wav'].to_host()), bits(want))
        assert np.array_equal(bits(c.run(pitch=0.0)['wav'].to_host()), bits(want))
        assert eng.profile_get('resample') == (0.0, 0) and eng.profile_get('stretch') == (0.0, 0)
        c.run(pitch=UP)
        assert eng.profile_get('resample')[1] == 1 and eng.profile_get('stretch')[1] == 1
    finally:
        eng.set_option('profile', 0)
    # the handle's setting, read when the call is made
    eng.set_pitch(UP)
    try:
        got = c.run()['wav'].to_host()
    finally:
        eng.set_pitch(0.0)
    assert np.array_equal(bits(got), bits(c.run(pitch=UP)['wav'].to_host())) and not np.array_equal(bits(got), bits(want))
    # refused settings leave the handle's as it was
    for bad in (float('nan'), float('inf'), 1.5, -1.01):
        assert eng.lib.tts_set_pitch(eng.handle, bad) == H.TTS_ERR_INVALID
    assert eng.lib.tts_set_pitch(None, 0.0) == H.TTS_ERR_INVALID
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(want))


@pytest.mark.parametrize('stop', [False, True], ids=['all-frames', 'end-of-speech'])
@pytest.mark.parametrize('octaves,s', [(UP, 1.0), (DOWN, 1.0), (UP, 1.2), (DOWN, 1.2)], ids=['up', 'down', 'up-rate1.2', 'down-rate1.2'])
def test_a_shifted_call_is_the_stage_calls_chained_by_hand(case, octaves, s, stop):
    c = case
    rate = None if s == 1.0 else s
    stop_arg = c.stop if stop else None
    plain = c.run(rate=rate, stop=stop_arg)                       # the same call without pitch: its shapes and lengths
    plain_frames = c.engine.synth_frames(c.B).tolist()
    out = c.run(pitch=octaves, rate=rate, stop=stop_arg, want=True)   # (the first call at this setting: not pipelined)
    wav = out['wav'].to_host()
    frames = c.engine.synth_frames(c.B).tolist()
    want, n_s, keep = c.chain(octaves, s, stop, peak=False)
    assert wav.shape == plain['wav'].shape == want.shape
    assert frames == plain_frames
    if stop:
        assert out['n_frames'].tolist() == plain['n_frames'].tolist() == n_s.tolist()
    print('octaves {:+.3f} rate {} stop {}: frames {}, samples kept {}'.format(octaves, s, stop, frames, keep))
    assert np.array_equal(bits(wav), bits(want))
    for b in range(c.B):
        assert not wav[b, keep[b]:].any() and not np.signbit(wav[b, keep[b]:]).any()
    # nothing else of the call moves
    for k in ('mel', 'alignments', 'linear'):
        assert np.array_equal(bits(out[k].to_host()), bits(c.off[k])), k
    # the same call again goes through the pipeline's streams, and unpipelined: the same bits
    assert np.array_equal(bits(c.run(pitch=octaves, rate=rate, stop=stop_arg)['wav'].to_host()), bits(wav))
    c.engine.set_option('pipeline', 0)
    try:
        assert np.array_equal(bits(c.run(pitch=octaves, rate=rate, stop=stop_arg)['wav'].to_host()), bits(wav))
    finally:
        c.engine.set_option('pipeline', 1)
    # peak normalisation runs on the resampled rows: the peak is 1 as in every other call
    peak = c.run(pitch=octaves, rate=rate, stop=stop_arg, peak=True)['wav'].to_host()
    want_peak, _n, _k = c.chain(octaves, s, stop, peak=True)
    assert np.array_equal(bits(peak), bits(want_peak))
    tops = np.abs(peak).max(axis=1)
    print('peaks', tops)
    assert (np.abs(tops.astype(np.float64) - 1.0) <= 2.0 ** -23).all()      # (x / x in the device's float32 division)


def test_host_form_is_the_device_form(case):
    c, cs = case, case.case
    eng = c.engine
    args = (cs['S'], E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'])
    want_plain = c.run(pitch=UP)['wav'].to_host()
    want_stop = c.run(pitch=UP, rate=1.2, stop=c.stop)
    want_stop_wav, want_n = want_stop['wav'].to_host(), want_stop['n_frames']
    t0 = eng.synthesize_host(E.ids_of(cs, seed=5), *args, seed=SEED, peak_normalize=False, pitch=UP)
    t1 = eng.synthesize_host(c.ids, *args, seed=SEED, peak_normalize=False, pitch=UP)
    t2 = eng.synthesize_host(c.ids, *args, seed=SEED, peak_normalize=False, pitch=UP, speaking_rate=1.2, stop_at_silence=c.stop)
    assert eng.wait_host(t0).shape == (c.B, c.hop * (c.T - 1))
    assert eng.wait_host_frames(t1).tolist() == [c.T] * c.B
    assert np.array_equal(bits(eng.wait_host(t1)), bits(want_plain))
    assert eng.wait_host_frames(t2).tolist() == want_n.tolist()
    got = eng.wait_host(t2)
    assert got.shape == want_stop_wav.shape and np.array_equal(bits(got), bits(want_stop_wav))
    off = eng.synthesize_host(c.ids, *args, seed=SEED, peak_normalize=False)
    assert np.array_equal(bits(eng.wait_host(off)), bits(c.off['wav']))


def test_settings_in_sequence_on_one_handle_are_the_fresh_handles_calls(case):
    """What a handle carries from call to call -- the plan's per-utterance lengths, the previous call's key, the buffers of the
    settings -- reaches no result: one handle taken through off, momentum, stopping, rate, pitch, all three and off again, every
    call made twice in a row (the first grows that setting's buffers, the second goes through the pipeline's streams), returns
    the waveforms and the frame counts, bit for bit, of a fresh handle that makes that one call."""
    c, cs = case, case.case
    settings = [('off', {}), ('momentum', dict(momentum=0.99)), ('stopping', dict(stop_at_silence=c.stop)),
                ('rate', dict(speaking_rate=1.2)), ('pitch', dict(pitch=UP)),
                ('all', dict(stop_at_silence=c.stop, speaking_rate=1.2, pitch=UP)), ('off', {})]

    def engine():
        eng = pkg().Engine(c.hp)
        eng.load_weights(E.weights_of(cs))
        return eng

    def call(eng, kw):
        out = eng.synthesize(c.ids, cs['S'], E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'], seed=SEED,
                             peak_normalize=False, **kw)
        return out['wav'].to_host(), eng.synth_frames(c.B).tolist()

    fresh = {}
    for name, kw in settings:
        if name not in fresh:
            eng = engine()
            try:
                fresh[name] = call(eng, kw)
            finally:
                eng.close()
    # the settings are six different calls
    assert fresh['off'][1] == fresh['momentum'][1] == fresh['pitch'][1] == [c.T] * c.B
    assert fresh['stopping'][1] == c.detected.tolist() and fresh['rate'][1] == [S.stretched_frames(c.T, 1.2)] * c.B
    assert fresh['all'][1] == c.lengths(1.2, S.stretched_frames(c.T, 1.2)).tolist()
    assert fresh['pitch'][0].shape == fresh['off'][0].shape and fresh['all'][0].shape == fresh['rate'][0].shape != fresh['off'][0].shape
    for name in ('momentum', 'stopping', 'pitch'):
        assert not np.array_equal(bits(fresh[name][0]), bits(fresh['off'][0])), name
    assert not np.array_equal(bits(fresh['all'][0]), bits(fresh['rate'][0]))
    eng = engine()
    try:
        for name, kw in settings:
            for nth in (1, 2):
                wav, frames = call(eng, kw)
                assert frames == fresh[name][1], (name, nth)
                assert wav.shape == fresh[name][0].shape and np.array_equal(bits(wav), bits(fresh[name][0])), (name, nth)
        assert eng._gl_momentum == 0 and eng._end_of_speech == (False, 0.0, 0) and eng._speaking_rate == 1.0 and eng._pitch == 0.0
    finally:
        eng.close()


def test_momentum_composes(case):
    c = case
    out = c.run(pitch=UP, momentum=0.99)['wav'].to_host()
    assert c.engine._gl_momentum == 0 and np.isfinite(out).all()
    assert out.shape == c.off['wav'].shape and not np.array_equal(out, c.run(pitch=UP)['wav'].to_host())


def test_a_product_outside_the_stretch_range_is_refused_at_the_call(case):
    """s * 2 ** -octaves outside [0.25, 4] is TTS_ERR_INVALID at the call: 2.5 * 2 = 5 and 0.4 / 2 = 0.2.  (2.5 with octaves = +1
    is 1.25 and legal: the product, not the pair, is what the stretch is given.)"""
    H = pkg('_hip')
    c, cs = case, case.case
    eng = c.engine
    args = (c.ids, cs['S'], E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'])
    for rate, octaves in [(2.5, -1.0), (0.4, 1.0)]:
        eng.set_speaking_rate(rate)
        eng.set_pitch(octaves)
        try:
            with pytest.raises(H.TtsError) as e:
                eng.synthesize(*args, seed=1, peak_normalize=False)
            assert e.value.code == H.TTS_ERR_INVALID and 'pitch' in str(e.value)
        finally:
            eng.set_pitch(0.0)
            eng.set_speaking_rate(1.0)
    # rows the call without pitch could not have either: 15 frames at rate 4 are 4 < min_frames = 5, though Griffin-Lim's
    # ceil(15 / (4 * 0.5)) = 8 would do; the message names the pitch
    with pytest.raises(H.TtsError) as e:
        eng.synthesize(c.ids, 3, E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'], seed=1, peak_normalize=False,
                       speaking_rate=4.0, pitch=1.0)
    assert e.value.code == H.TTS_ERR_INVALID and 'with a pitch' in str(e.value)
    out = c.run(pitch=1.0, rate=2.5)
    assert out['wav'].shape == (c.B, c.hop * (S.stretched_frames(c.T, 2.5) - 1)) and np.isfinite(out['wav'].to_host()).all()
    assert np.array_equal(bits(c.run()['wav'].to_host()), bits(c.off['wav']))


def test_engine_pitch_shift(engine):
    """a two-tone signal shifted one octave up: the spectral peak moves to twice its frequency, the length stays"""
    n = 4096
    t = np.arange(n)
    x = (0.6 * np.sin(2 * np.pi * 200.0 * t / n) + 0.2 * np.sin(2 * np.pi * 330.0 * t / n)).astype(np.float32)
    y = engine.pitch_shift(x, 22050, 1.0, seed=3)
    assert y.shape == (n,)
    y = y.to_host()
    assert np.isfinite(y).all()
    peak_in = int(np.argmax(np.abs(np.fft.rfft(x * np.hanning(n)))))
    peak_out = int(np.argmax(np.abs(np.fft.rfft(y * np.hanning(n)))))
    print('spectral peak: bin {} -> bin {}'.format(peak_in, peak_out))
    assert peak_in == 200 and abs(peak_out - 2 * peak_in) <= 1
    both = engine.pitch_shift(np.stack([x, x[::-1].copy()]), 22050, -0.5, n_iter=2, seed=3)
    assert both.shape == (2, n)


# ---------------------------------------------------------------------------------------------- the Python surface on the device
def test_serve_post_processing_shifts_with_the_stage_calls(case, monkeypatch):
    """tacotron.serve.post_process_spectrograms(pitch=..., stop_at_silence_db=...): the lengths of the engine's shifted call, and
    bit for bit the stage calls it is made of chained by hand -- tts_denorm_power, tts_stretch_magnitudes at rate * rho, the
    ragged Griffin-Lim on the lengths at that rate, tts_resample by rho into rows of the call without pitch, cut where that
    call's utterances end"""
    V = pkg('tacotron.serve')
    P = pkg('tacotron.params')
    c, eng, cs = case, case.engine, case.case
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', cs['n_iter'])
    loader = P.dataset_params.dataset_loader
    linear = c.off['linear']
    for octaves, s in [(UP, 1.2), (DOWN, 1.0)]:
        rho = float(np.exp2(-np.float64(octaves)))
        eff = s * rho
        Tg = S.stretched_frames(c.T, eff)
        Tw = c.T if s == 1.0 else S.stretched_frames(c.T, s)
        wavs = V.post_process_spectrograms(linear, eng, seed=SEED, stop_at_silence_db=float(c.threshold_db), silence_keep_ms=0.0,
                                           speaking_rate=s, pitch=octaves)
        piped = c.run(pitch=octaves, rate=None if s == 1.0 else s, stop=c.stop)
        n_s = piped['n_frames']
        assert n_s.tolist() == c.lengths(s, Tw).tolist()
        assert [len(w) for w in wavs] == [c.hop * (int(n) - 1) for n in n_s]
        mag = eng.denorm_power(linear, loader.mel_mag_ref_db, loader.mel_mag_max_db, P.model_params.magnitude_power)
        st = eng.stretch_magnitudes(mag, eff, n_frames=c.detected, T_out=Tg)
        n_gl = c.lengths(eff, Tg)
        gl, _ = eng.griffin_lim(st, cs['n_iter'], cs['win'], cs['hop'], cs['n_fft'], seed=SEED, want_mse=False, n_frames=n_gl)
        want = eng.resample(gl, rho, n_samples=c.hop * (n_gl - 1), N_out=c.hop * (Tw - 1)).to_host()
        for b, w in enumerate(wavs):
            assert np.array_equal(bits(w), bits(want[b, :len(w)])), (octaves, s, b)
            assert np.abs(w).max() > 0
        # ... and it is the engine's call to rounding: the same samples are silent, the same loud
        got = piped['wav'].to_host()
        for b, w in enumerate(wavs):
            err = np.linalg.norm(w.astype(np.float64) - got[b, :len(w)]) / np.linalg.norm(got[b, :len(w)])
            print('serve octaves {:+.3f} rate {} b={}: rel-L2 against the call pipeline {:.2e}'.format(octaves, s, b, err))
    # without stopping: every waveform has the length of the call without pitch
    plain = V.post_process_spectrograms(linear, eng, seed=SEED, speaking_rate=1.2, pitch=UP)
    assert [len(w) for w in plain] == [c.hop * (S.stretched_frames(c.T, 1.2) - 1)] * c.B


def test_pitch_through_the_inference_helpers(case):
    """pitch= through tacotron.inference.synthesize_batch and synthesize_stream (three host calls in flight): the bits of
    Engine.synthesize with the same setting"""
    Inf = pkg('tacotron.inference')
    Tm = pkg('tacotron.model')
    c, cs = case, case.case
    model = Tm.Tacotron(inputs=Tm.Tacotron.model_placeholders(), mode=Tm.Mode.PREDICT, engine=c.engine, hparams=c.hp)
    wavs = Inf.synthesize_batch(model, c.ids, n_steps=cs['S'], n_iter=cs['n_iter'], seed=SEED, pitch=UP)
    assert np.array_equal(bits(wavs), bits(c.run(pitch=UP)['wav'].to_host()))
    got = [w.copy() for w in Inf.synthesize_stream(model, iter([c.ids] * 4), n_steps=cs['S'], n_iter=cs['n_iter'], seed=SEED,
                                                   speaking_rate=1.2, pitch=DOWN)]
    assert len(got) == 4
    for k, w in enumerate(got):
        assert np.array_equal(bits(w), bits(c.run(pitch=DOWN, rate=1.2, seed=SEED + k)['wav'].to_host())), k
    assert c.engine._pitch == 0.0 and c.engine._speaking_rate == 1.0
    cut = Inf.synthesize_batch(model, c.ids, n_steps=cs['S'], n_iter=cs['n_iter'], seed=SEED, pitch=UP,
                               stop_at_silence_db=float(c.threshold_db), silence_keep_ms=0.0)
    want = c.run(pitch=UP, stop=c.stop)
    assert [len(w) for w in cut] == [c.hop * (int(n) - 1) for n in want['n_frames']]
    for b, w in enumerate(cut):
        assert np.array_equal(bits(w), bits(want['wav'].to_host()[b, :len(w)])), b


def test_audio_io_resample_is_engine_resample(engine):
    """audio.io.resample(wav, orig_sr, target_sr) = librosa.core.resample(fix=True, scale=False): Engine.resample at
    target_sr / orig_sr, ceil(n * ratio) samples, the input's float type; and a 1-D device buffer is one waveform"""
    io = pkg('audio.io')
    x = np.random.default_rng(8).standard_normal(3000).astype(np.float32)
    rho = 16000.0 / 22050.0
    y = io.resample(x, 22050, 16000, engine=engine)
    d = engine.resample(x, rho)
    want = d.to_host()
    d.free()
    assert y.dtype == np.float32 and y.shape == want.shape == (R.resampled_length(3000, rho),)
    assert np.array_equal(bits(y), bits(want))
    y64, sabs = R.resample(x.astype(np.float64), rho)
    assert (np.abs(y.astype(np.float64) - y64) <= R.bound(y64, sabs)).all()
    assert not y[R.resampled_valid(3000, rho):].any()
    up = io.resample(x.astype(np.float64), 16000, 22050, engine=engine)
    assert up.dtype == np.float64 and up.shape == (R.resampled_length(3000, 22050.0 / 16000.0),)
    dx = engine.to_device(x)
    one = engine.resample(dx, rho)
    assert one.shape == want.shape and np.array_equal(bits(one.to_host()), bits(want))
    one.free()
    dx.free()
