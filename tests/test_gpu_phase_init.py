"""GPU: estimated initial phases for Griffin-Lim (csrc/phase_init.hip).  tts_phase_estimate equals the sequential oracle
(tests/phase_oracle.py) bit for bit in both input layouts; the option "gl_init" = 1 gives the bits of the same call handed the
estimate of its own magnitudes as an explicit init_phase, in tts_griffin_lim, tts_griffin_lim_ragged and tts_synthesize; and
the quality statement of the host test holds on the device.

Shapes: one bin count per row width (129, 1025, 2049 bins), frame counts at both sides of the kernel's chunk length and over
two chunks, B = 8 (one kind of input per utterance) and ragged batches of three."""
import ctypes

import numpy as np
import pytest

import eos_cases as E
import momentum_oracle as M
import phase_cases as K
import phase_oracle as P
import stretch_oracle as S
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_ORACLE = {}


def batch_of_kinds(n_fft, T):
    """(mag (8, F, T), the oracle's init_phase (8, F, T)): every kind of input side by side, computed once per shape"""
    key = (n_fft, T)
    if key not in _ORACLE:
        mag = np.stack([K.magnitudes(kind, n_fft, T) for kind in K.KINDS])
        _ORACLE[key] = (mag, P.phase_estimate(mag, n_fft, K.HOP[n_fft]))
    return _ORACLE[key]


def shapes(chunk):
    return [(n_fft, T) for n_fft in (256, 2048, 4096) for T in K.frame_counts(n_fft, chunk)]


def _chunk():
    return int(pkg('_hip').load_library().tts_phase_chunk_frames())


def _report(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    print('{}: {} of {} values differ{}'.format(what, int(bad.sum()), bad.size,
                                               '' if not bad.any() else ', first at (b, k, t) = {}'.format(tuple(int(v[0]) for v in np.nonzero(bad)))))


@pytest.mark.parametrize('n_fft,T', shapes(_chunk()), ids=lambda v: str(v))
def test_the_estimate_equals_the_oracle_bit_for_bit_in_both_layouts(engine, n_fft, T):
    mag, want = batch_of_kinds(n_fft, T)
    hop, F = K.HOP[n_fft], 1 + n_fft // 2
    got = engine.phase_estimate(mag, n_fft, hop)
    rows = np.ascontiguousarray(mag.transpose(0, 2, 1))
    got_rows = engine.phase_estimate_rows(rows, n_fft, hop)                                   # rows F floats apart
    got_padded = engine.phase_estimate_rows(rows, n_fft, hop, row_stride=(F + 31) // 32 * 32)    # the pipeline's rows, NaN padding
    try:
        for name, g in (('public', got), ('rows', got_rows), ('padded rows', got_padded)):
            g = g.to_host()
            _report(g, want, '{} n_fft {} T {}'.format(name, n_fft, T))
            for b, kind in enumerate(K.KINDS):
                assert np.array_equal(g[b], want[b]), (name, kind)
    finally:
        for g in (got, got_rows, got_padded):
            g.free()


@pytest.mark.parametrize('n_fft,T', [(256, 41), (2048, 33), (2048, 67)], ids=lambda v: str(v))
def test_ragged_batches_read_and_write_nothing_behind_an_utterances_end(engine, n_fft, T):
    """NaN behind every end in the input (never read: the results are finite and the oracle's), a sentinel behind every end in
    the output (never written)"""
    H = pkg('_hip')
    mag, n = K.ragged_batch(n_fft, T)
    hop, F = K.HOP[n_fft], 1 + n_fft // 2
    want = P.phase_estimate(mag, n_fft, hop, n_frames=n, fill=SENTINEL)
    assert np.isfinite(want).all()
    d_mag = engine.to_device(mag)
    stride = (F + 31) // 32 * 32
    rows = np.full((3, T, stride), np.nan, np.float32)
    rows[:, :, :F] = mag.transpose(0, 2, 1)
    d_rows = engine.to_device(rows)
    p_n = n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    try:
        for name in ('public', 'rows'):
            out = engine.to_device(np.full((3, F, T), SENTINEL, np.float32))
            if name == 'public':
                rc = engine.lib.tts_phase_estimate(engine.handle, d_mag.data_ptr(), 3, T, p_n, n_fft, hop, out.data_ptr())
            else:
                rc = engine.lib.tts_phase_estimate_rows(engine.handle, d_rows.data_ptr(), 3, T, stride, p_n, n_fft, hop, out.data_ptr())
            assert rc == H.TTS_OK
            got = out.to_host()
            out.free()
            _report(got, want, '{} ragged n_fft {} T {}'.format(name, n_fft, T))
            assert np.array_equal(got, want), name
        # an utterance's phases do not depend on the batch it is in
        alone = engine.phase_estimate(np.ascontiguousarray(mag[2:3, :, :n[2]]), n_fft, hop)
        assert np.array_equal(alone.to_host()[0], want[2, :, :n[2]])
        alone.free()
    finally:
        d_mag.free()
        d_rows.free()


def test_the_library_refuses_bad_arguments_and_option_values(engine):
    H = pkg('_hip')
    lib, h = engine.lib, engine.handle
    d = engine.to_device(np.ones((2, 129, 4), np.float32))
    out = engine.to_device(np.full((2, 129, 4), SENTINEL, np.float32))
    good = np.array([4, 2], np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    try:
        calls = [(None, 2, 4, None, 256, 64, out.data_ptr()), (d.data_ptr(), 2, 4, None, 256, 64, None),
                 (d.data_ptr(), 0, 4, None, 256, 64, out.data_ptr()), (d.data_ptr(), 2, 0, None, 256, 64, out.data_ptr()),
                 (d.data_ptr(), 2, 4, None, 250, 64, out.data_ptr()), (d.data_ptr(), 2, 4, None, 8192, 64, out.data_ptr()),
                 (d.data_ptr(), 2, 4, None, 256, 0, out.data_ptr()), (d.data_ptr(), 2, 4, None, 256, 257, out.data_ptr()),
                 (d.data_ptr(), 2, 4, ptr(np.array([4, 0], np.int32)), 256, 64, out.data_ptr()),
                 (d.data_ptr(), 2, 4, ptr(np.array([5, 1], np.int32)), 256, 64, out.data_ptr())]
        for args in calls:
            assert lib.tts_phase_estimate(h, *args) == H.TTS_ERR_INVALID, args
        assert lib.tts_phase_estimate_rows(h, d.data_ptr(), 2, 4, 128, None, 256, 64, out.data_ptr()) == H.TTS_ERR_INVALID
        engine.synchronize()
        assert (out.to_host() == SENTINEL).all()                 # nothing was enqueued
        assert lib.tts_phase_estimate(h, d.data_ptr(), 2, 4, ptr(good), 256, 64, out.data_ptr()) == H.TTS_OK
        # the option: 0 and 1, anything else is refused and leaves it as it was
        mag = K.magnitudes('fixture', 2048, 12)[None]
        engine.set_option('gl_init', 1)
        try:
            on = engine.griffin_lim(mag, 2, 1102, 275, 2048, seed=3)[0].to_host()
            for bad in (2, -1, 1000):
                assert lib.tts_set_option(h, b'gl_init', bad) == H.TTS_ERR_INVALID
            assert np.array_equal(bits(engine.griffin_lim(mag, 2, 1102, 275, 2048, seed=4)[0].to_host()), bits(on))   # still on: the seed is unused
        finally:
            engine.set_option('gl_init', 0)
        off = engine.griffin_lim(mag, 2, 1102, 275, 2048, seed=3)[0].to_host()
        assert not np.array_equal(bits(off), bits(on))
        assert engine._gl_init == 0
    finally:
        d.free()
        out.free()


# ---------------------------------------------------------------------------------------------- Griffin-Lim with the option
GL_CASES = {'streaming': (2048, 1102, 275, 12), 'general-512': (512, 400, 100, 12)}


def _gl_mag(n_fft, T):
    return np.stack([K.magnitudes('fixture', n_fft, T), K.magnitudes('chirp', n_fft, T) + np.float32(0.01), K.magnitudes('random', n_fft, T)])


@pytest.mark.parametrize('options', [{}, {'gl_momentum': 990}, {'gl_pair': 1}], ids=['plain', 'momentum', 'pair1'])
@pytest.mark.parametrize('ragged', [False, True], ids=['uniform', 'ragged'])
@pytest.mark.parametrize('case', sorted(GL_CASES))
def test_griffin_lim_with_the_option_is_the_call_given_the_estimate(engine, case, ragged, options):
    n_fft, win, hop, T = GL_CASES[case]
    mag = _gl_mag(n_fft, T)
    n = np.array([T, 7, 9], np.int32) if ragged else None
    saved = {'gl_momentum': 0, 'gl_pair': 3}
    for k, v in options.items():
        engine.set_option(k, v)
    try:
        est = engine.phase_estimate(mag, n_fft, hop, n_frames=n)
        want_est = P.phase_estimate(mag, n_fft, hop, n_frames=n)
        g = est.to_host()
        for b in range(3):
            nb = T if n is None else int(n[b])
            assert np.array_equal(g[b, :, :nb], want_est[b, :, :nb])
        for n_iter in (2, 0):
            wav_on, mse_on = engine.griffin_lim(mag, n_iter, win, hop, n_fft, seed=5, n_frames=n, phase_init='estimate')
            wav_by_hand, mse_by_hand = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=est, seed=5, n_frames=n, phase_init='random')
            wav_random, _ = engine.griffin_lim(mag, n_iter, win, hop, n_fft, seed=5, n_frames=n, phase_init='random')
            a, b_, r = wav_on.to_host(), wav_by_hand.to_host(), wav_random.to_host()
            assert np.isfinite(a).all()
            assert np.array_equal(bits(a), bits(b_)), n_iter
            assert np.array_equal(bits(mse_on.to_host()), bits(mse_by_hand.to_host())), n_iter
            assert not np.array_equal(bits(a), bits(r)), n_iter        # (the option did something)
            # an explicit init_phase always wins
            wav_both, _ = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=est, seed=5, n_frames=n, phase_init='estimate')
            assert np.array_equal(bits(wav_both.to_host()), bits(b_))
            for w in (wav_on, wav_by_hand, wav_random, wav_both, mse_on, mse_by_hand):
                w.free()
        assert engine._gl_init == 0
        est.free()
    finally:
        for k in options:
            engine.set_option(k, saved[k])


def test_quality_on_the_device(engine):
    """the host statement (frames 100:260 of the shipped spectrogram) through tts_griffin_lim's mse: 20 iterations from the
    estimate are at or below 60 from default_rng(0) phases, and the first iteration is below a quarter of the random start's.
    Host oracle: 9.40e-6 against 1.341e-5, 3.94e-5 against 4.21e-4."""
    mag, init = M.shipped_spectrogram(100, 260)
    run = lambda n_iter, **kw: float(engine.griffin_lim(mag[None], n_iter, 1102, 275, 2048, **kw)[1].to_host()[0])
    rand1, rand60 = run(1, init_phase=init[None]), run(60, init_phase=init[None])
    est1, est20 = run(1, phase_init='estimate'), run(20, phase_init='estimate')
    print('random: 1 {:.3e}, 60 {:.3e};  estimate: 1 {:.3e}, 20 {:.3e}'.format(rand1, rand60, est1, est20))
    assert est20 <= rand60
    assert est1 < 0.25 * rand1
    # the Python mirror of the reference's function states the start of every call
    Y = pkg('audio.synthesis')
    _w, mse = Y.griffin_lim_v2(mag, 1102, 275, 2048, 20, engine=engine, phase_init='estimate')
    assert float(mse) == est20


# ---------------------------------------------------------------------------------------------- tts_synthesize
SEED = 9
UP = 4.0 / 12.0


class Synth(object):
    """the small end-to-end case of eos_cases.py on a handle of its own (B = 3, T = 40 frames of 275 samples, 3 iterations)"""

    def __init__(self, case):
        self.case = case
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.B, self.T = case['B'], case['S'] * self.hp.reduction
        self.hop, self.n_fft, self.F = case['hop'], case['n_fft'], 1 + case['n_fft'] // 2
        self.FP = (self.F + 31) // 32 * 32
        off = self.run(want=True)                     # on a handle that never had the option on
        self.off = off['wav'].to_host()
        self.threshold_db = E.choose_threshold(off['linear'].to_host(), case['min_frames'])
        assert self.threshold_db is not None
        self.stop = (self.threshold_db, 0)
        self.detected = self.run(stop=self.stop)['n_frames']
        self.off_stop = self.run(stop=self.stop)['wav'].to_host()

    def run(self, phase_init=None, init=None, rate=None, stop=None, pitch=None, want=False, seed=SEED):
        c = self.case
        return self.engine.synthesize(self.ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'], init_phase=init,
                                      seed=seed, peak_normalize=False, want_linear=want, stop_at_silence=stop, speaking_rate=rate,
                                      pitch=pitch, phase_init=phase_init)

    def own_estimate(self, rate, pitch, stop):
        """tts_phase_estimate of the magnitudes the last call's Griffin-Lim reconstructed from, at the lengths it ran on"""
        eff = (1.0 if rate is None else rate) * float(np.exp2(-np.float64(0.0 if pitch is None else pitch)))
        stretch = rate is not None or pitch is not None
        Tg = S.stretched_frames(self.T, eff) if stretch else self.T
        rows = self.engine.debug_workspace('gl.mag_st' if stretch else 'gl.mag', (self.B, Tg, self.FP))
        mag = np.ascontiguousarray(rows[:, :, :self.F].transpose(0, 2, 1))
        n = None
        if stop:
            n = S.stretched_lengths(self.detected, eff, Tg, self.case['min_frames']) if stretch else self.detected.copy()
            for b in range(self.B):
                mag[b, :, n[b]:] = np.nan      # (whatever the buffer holds there, it must not matter)
        return self.engine.phase_estimate(mag, self.n_fft, self.hop, n_frames=n), n


@pytest.fixture(scope='module')
def synth():
    s = Synth(E.E2E)
    yield s
    s.engine.close()


@pytest.mark.parametrize('setting', ['alone', 'rate1.25', 'end-of-speech', 'pitch-up', 'end-of-speech-rate1.25'])
def test_synthesize_with_the_option_is_the_call_given_the_estimate_of_its_own_magnitudes(synth, setting):
    s, eng = synth, synth.engine
    rate = 1.25 if 'rate' in setting else None
    stop = s.stop if 'end-of-speech' in setting else None
    pitch = UP if 'pitch' in setting else None
    kw = dict(rate=rate, stop=stop, pitch=pitch)
    first = s.run(phase_init='estimate', **kw)['wav'].to_host()         # (the option is new to this shape: not pipelined)
    assert np.isfinite(first).all()
    est, n = s.own_estimate(rate, pitch, stop)
    second = s.run(phase_init='estimate', seed=SEED + 1, **kw)['wav'].to_host()   # pipelined; the seed is unused
    assert np.array_equal(bits(second), bits(first))
    want = s.run(phase_init='random', init=est, **kw)['wav'].to_host()
    assert want.shape == first.shape
    assert np.array_equal(bits(first), bits(want))
    assert np.array_equal(bits(s.run(phase_init='estimate', init=est, **kw)['wav'].to_host()), bits(want))   # explicit wins
    random = s.run(phase_init='random', **kw)['wav'].to_host()
    assert not np.array_equal(bits(random), bits(first))
    eng.set_option('pipeline', 0)
    try:
        assert np.array_equal(bits(s.run(phase_init='estimate', **kw)['wav'].to_host()), bits(first))
        assert np.array_equal(bits(s.run(phase_init='random', init=est, **kw)['wav'].to_host()), bits(first))
    finally:
        eng.set_option('pipeline', 1)
    # the handle's option, read when the call is made
    eng.set_option('gl_init', 1)
    try:
        assert np.array_equal(bits(s.run(**kw)['wav'].to_host()), bits(first))
    finally:
        eng.set_option('gl_init', 0)
    est.free()
    # option off afterwards: the bits of the handle that never had it on
    assert eng._gl_init == 0
    assert np.array_equal(bits(s.run()['wav'].to_host()), bits(s.off))
    assert np.array_equal(bits(s.run()['wav'].to_host()), bits(s.off))
    assert np.array_equal(bits(s.run(stop=s.stop)['wav'].to_host()), bits(s.off_stop))


def test_the_estimate_has_a_profile_stage_and_off_launches_nothing(synth):
    s, eng = synth, synth.engine
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(s.run()['wav'].to_host()), bits(s.off))
        assert np.array_equal(bits(s.run(phase_init='random')['wav'].to_host()), bits(s.off))
        assert eng.profile_get('phase_init') == (0.0, 0)
        s.run(phase_init='estimate')
        ms, launches = eng.profile_get('phase_init')
        assert launches == 4                       # 40 frames are two chunks: compose, chain, apply, transpose
    finally:
        eng.set_option('profile', 0)


def test_host_form_is_the_device_form(synth):
    s, cs, eng = synth, synth.case, synth.engine
    args = (cs['S'], E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'])
    want = s.run(phase_init='estimate')['wav'].to_host()
    want_stop = s.run(phase_init='estimate', stop=s.stop)['wav'].to_host()
    t0 = eng.synthesize_host(E.ids_of(cs, seed=5), *args, seed=SEED, peak_normalize=False, phase_init='estimate')
    t1 = eng.synthesize_host(s.ids, *args, seed=SEED, peak_normalize=False, phase_init='estimate')
    t2 = eng.synthesize_host(s.ids, *args, seed=SEED, peak_normalize=False, phase_init='estimate', stop_at_silence=s.stop)
    eng.wait_host(t0)
    assert np.array_equal(bits(eng.wait_host(t1)), bits(want))
    assert np.array_equal(bits(eng.wait_host(t2)), bits(want_stop))
    assert np.array_equal(bits(s.run()['wav'].to_host()), bits(s.off))


def test_general_kernels_take_the_option_too():
    s = Synth(E.E2E_512)
    try:
        first = s.run(phase_init='estimate')['wav'].to_host()
        est, _n = s.own_estimate(None, None, None)
        assert np.array_equal(bits(s.run(phase_init='random', init=est)['wav'].to_host()), bits(first))
        assert np.array_equal(bits(s.run(phase_init='estimate')['wav'].to_host()), bits(first))
        assert np.array_equal(bits(s.run()['wav'].to_host()), bits(s.off))
        est.free()
    finally:
        s.engine.close()
