"""GPU: the speaking rate -- the two stretch kernels (tts_stretch_magnitudes, reference layout; tts_stretch_rows, time-major
padded rows) against the oracle's round-once blend (tests/stretch_oracle.py, a restatement of what the reference's
time_stretch, audio/effects.py:46-88, hands to Griffin-Lim) by exact bit equality, and the setting inside tts_synthesize /
tts_synthesize_host: the waveform is the Griffin-Lim oracle's reconstruction of the stretched oracle magnitudes, the lengths
with end-of-speech stopping are min(T', max(min_frames, ceil(n / rate))), and nothing else of the call moves.

Shapes: B = 3, T = 12 for the kernels (F = 1025: rows at every alignment; 129: one 16-byte load and a tail; 1), lengths
[12, 7, 1]; end to end the cases of eos_cases.py (T = 40 in the streaming kernel, T = 25 in the general kernels)."""
import ctypes

import numpy as np
import pytest

import audio_cases as C
import eos_cases as E
import momentum_oracle as M
import stretch_cases as K
import stretch_oracle as S
from conftest import pkg
from oracle import audio_oracle as A
from parity import assert_parity, assert_segment_parity

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cols(engine, x, rate, n_frames=None, T_out=None):
    d = engine.stretch_magnitudes(x, rate, n_frames=n_frames, T_out=T_out)
    out = d.to_host()
    d.free()
    return out


def _rows(engine, x_ft, rate, n_frames=None, T_out=None, pad=K.PAD):
    """the time-major kernel on x (B, F, T): rows of F + pad floats, NaN in the padding; returns (B, F, T_out) again"""
    F = x_ft.shape[1]
    full = K.time_major(x_ft, pad)
    d = engine.stretch_rows(full[:, :, :F] if pad else full, rate, n_frames=n_frames, T_out=T_out, row_stride=F + pad)
    out = d.to_host()[:, :, :F]
    d.free()
    return np.ascontiguousarray(out.transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('ragged', [True, False], ids=['ragged', 'uniform'])
@pytest.mark.parametrize('F', K.STAGE_F)
def test_both_layouts_equal_the_oracle_bit_for_bit(engine, F, ragged):
    x = K.stage_batch(F)
    nf = K.STAGE_LENGTHS if ragged else None
    dirty = K.poisoned(x, nf)     # NaN in every column behind an utterance's length: it must never be read
    for rate in K.STAGE_RATES:
        for extra in (0, 3):
            T_out = K.longest(nf, K.STAGE_T, rate) + extra
            want = S.blend_batch(x, rate, nf, T_out)
            label = (F, ragged, rate, T_out)
            cols = _cols(engine, dirty, rate, nf, T_out)
            rows = _rows(engine, dirty, rate, nf, T_out)
            assert cols.shape == rows.shape == want.shape == (K.STAGE_B, F, T_out), label
            assert not np.isnan(cols).any() and not np.isnan(rows).any(), label
            assert np.array_equal(bits(cols), bits(want)), label
            assert np.array_equal(bits(rows), bits(cols)), label            # the two layouts: the same bits
            for b in range(K.STAGE_B):                                       # the tail of every row is +0.0
                m = S.stretched_frames(nf[b] if ragged else K.STAGE_T, rate)
                assert not bits(cols[b, :, m:]).any() and not bits(rows[b, :, m:]).any(), label
    if not ragged:   # rate 1.0 is a legal direct call: the input bits
        assert np.array_equal(bits(_cols(engine, x, 1.0)), bits(x)) and np.array_equal(bits(_rows(engine, x, 1.0)), bits(x))


def test_unaligned_rows_take_the_scalar_path(engine):
    """row_stride = F + 2 (not a multiple of 4) and no padding at all: the same bits as the 16-byte path"""
    x = K.stage_batch(129)
    for rate in (0.75, 1.3):
        want = S.blend_batch(x, rate, K.STAGE_LENGTHS)
        for pad in (2, 0):
            assert np.array_equal(bits(_rows(engine, K.poisoned(x, K.STAGE_LENGTHS), rate, K.STAGE_LENGTHS, pad=pad)), bits(want)), (rate, pad)


@pytest.mark.parametrize('rate', [2.0, 1.3])
def test_non_finite_inputs_behave_as_in_numpy(engine, rate):
    """rate 2.0: frame k reads columns 2k (a = 0) and 2k + 1 with weight 0 -- a NaN or +Inf in an odd column reaches the output
    through 0 * x alone and must make it NaN; rate 1.3 hits the same columns with a != 0"""
    F = 129
    x = K.stage_batch(F)[:1]
    bad = x.copy()
    bad[0, 5, 3] = np.nan
    bad[0, 7, 5] = np.inf
    bad[0, 9, 4] = np.inf
    want_clean, want = S.blend_batch(x, rate), S.blend_batch(bad, rate)
    if rate == 2.0:   # the weight-zero neighbours: NaN from 0 * NaN and from 0 * Inf; an Inf read with weight one stays Inf
        assert np.isnan(want[0, 5, 1]) and np.isnan(want[0, 7, 2]) and np.isposinf(want[0, 9, 2])
    else:
        assert np.isnan(want[0, 5]).sum() >= 1 and np.isposinf(want[0, 7]).sum() >= 1
    touched = bits(want) != bits(want_clean)
    touched |= np.isnan(want)
    for run in (_cols, _rows):
        clean, got = run(engine, x, rate), run(engine, bad, rate)
        assert np.array_equal(np.isnan(got), np.isnan(want)), run.__name__
        assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)]), run.__name__
        assert np.array_equal(bits(got)[~touched], bits(clean)[~touched]), run.__name__   # every other element: the clean run's bits
        assert np.array_equal(bits(clean), bits(want_clean))


@pytest.mark.parametrize('F', [1025, 1])
def test_an_utterance_does_not_depend_on_its_batch(engine, F):
    x = K.poisoned(K.stage_batch(F), K.STAGE_LENGTHS)
    nf = K.STAGE_LENGTHS
    rate, T_out = 1.3, K.longest(nf, K.STAGE_T, 1.3)
    for run in (_cols, _rows):
        whole = run(engine, x, rate, nf, T_out)
        rev = run(engine, np.ascontiguousarray(x[::-1]), rate, nf[::-1], T_out)
        assert np.array_equal(bits(rev), bits(whole[::-1]))
        for b in range(K.STAGE_B):
            one = run(engine, x[b:b + 1], rate, nf[b:b + 1], T_out)
            assert np.array_equal(bits(one[0]), bits(whole[b])), (run.__name__, b)


def test_more_utterances_than_one_launch_takes(engine):
    """B = 70: the lengths travel 64 utterances per launch"""
    rng = np.random.default_rng(70)
    B, F, T = 70, 5, 9
    x = rng.random((B, F, T)).astype(np.float32)
    nf = rng.integers(1, T + 1, B).tolist()
    want = S.blend_batch(x, 0.75, nf)
    assert np.array_equal(bits(_cols(engine, K.poisoned(x, nf), 0.75, nf)), bits(want))
    assert np.array_equal(bits(_rows(engine, K.poisoned(x, nf), 0.75, nf)), bits(want))
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        _cols(engine, x, 0.75, nf)
        assert engine.profile_get('stretch')[1] == 2
    finally:
        engine.set_option('profile', 0)


def test_refusals_leave_the_output_untouched(engine):
    H = pkg('_hip')
    B, F, T = 3, 5, 12
    mag = engine.to_device(np.ones((B, F, T), np.float32))
    out = engine.to_device(np.full((B, F + 3, 30), -7.0, np.float32))
    lens = (ctypes.c_int32 * B)(12, 7, 1)
    pm, po = mag.data_ptr(), out.data_ptr()
    cols = lambda *a: engine.lib.tts_stretch_magnitudes(engine.handle, *a)   # noqa: E731
    rows = lambda *a: engine.lib.tts_stretch_rows(engine.handle, *a)         # noqa: E731
    nan, inf = float('nan'), float('inf')

    def lens_with(b, v):
        a = (ctypes.c_int32 * B)(12, 7, 1)
        a[b] = v
        return a

    try:
        bad = [(pm, B, F, T, lens, r, 30, po) for r in (nan, inf, 0.0, 0.2, 4.5, -1.0)]
        bad += [(pm, 0, F, T, None, 1.3, 30, po), (pm, B, 0, T, None, 1.3, 30, po), (pm, B, F, 0, None, 1.3, 30, po)]
        bad += [(pm, B, F, T, lens_with(1, v), 1.3, 30, po) for v in (0, -1, T + 1)]
        bad += [(pm, B, F, T, lens, 1.3, 9, po), (pm, B, F, T, None, 0.5, 23, po), (None, B, F, T, lens, 1.3, 30, po), (pm, B, F, T, lens, 1.3, 30, None)]
        for args in bad:
            assert cols(*args) == H.TTS_ERR_INVALID, args
            assert rows(args[0], args[1], args[3], args[2], args[2], *args[4:]) == H.TTS_ERR_INVALID, args   # (B, T, F, row_stride)
        assert rows(pm, B, T, F, F - 1, lens, 1.3, 30, po) == H.TTS_ERR_INVALID
        assert engine.lib.tts_stretch_magnitudes(None, pm, B, F, T, lens, 1.3, 30, po) == H.TTS_ERR_INVALID
        engine.synchronize()
        assert np.array_equal(out.to_host(), np.full((B, F + 3, 30), -7.0, np.float32))
        with pytest.raises(H.TtsError) as e:
            engine._check(cols(pm, B, F, T, lens, 1.3, 9, po))
        assert 'T_out' in str(e.value)
        assert cols(pm, B, F, T, lens, 1.3, 10, po) == H.TTS_OK
    finally:
        mag.free()
        out.free()


def test_profile_stage_reports_its_launches(engine):
    x = K.stage_batch(129)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        _cols(engine, x, 1.3)
        ms1, n1 = engine.profile_get('stretch')
        _rows(engine, x, 1.3)
        ms2, n2 = engine.profile_get('stretch')
    finally:
        engine.set_option('profile', 0)
    assert (n1, n2) == (1, 2) and 0 < ms1 <= ms2
    assert engine.stretched_frames(12, 1.3) == 10 and engine.stretched_frames(40, 0.8) == 50


# ---------------------------------------------------------------------------------------------- end to end
RATES = [1.25, 0.8]


class Case(object):
    """an engine of the case's architecture, the rate-1.0 call (made once, on a handle whose rate was never set) and what
    the tests derive from it"""

    def __init__(self, case):
        self.case = case
        self.hp = E.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.load_weights(E.weights_of(case))
        self.ids = E.ids_of(case)
        self.T = case['S'] * self.hp.reduction
        self.hop, self.F = case['hop'], 1 + case['n_fft'] // 2
        self.init1 = E.init_of(case)
        off = self.run(None, want=True)
        self.off = {k: off[k].to_host() for k in ('wav', 'mel', 'linear', 'alignments')}
        self.linear = self.off['linear']
        self.mag = [A.linear_to_magnitude(self.linear[b], E.REF_DB, E.MAX_DB, E.POWER) for b in range(case['B'])]   # (F, T) float64
        self.threshold_db = E.choose_threshold(self.linear, case['min_frames'])
        assert self.threshold_db is not None, 'no gap between the frame maxima gives three different lengths'
        self.lengths = E.oracle_lengths(self.linear, self.threshold_db, 0, case['min_frames'])
        self._ref = {}

    def Tg(self, rate):
        return self.T if rate in (None, 1.0) else S.stretched_frames(self.T, rate)

    def init(self, rate):
        if rate in (None, 1.0):
            return self.init1
        return np.random.default_rng(17).random((self.case['B'], self.F, self.Tg(rate))).astype(np.float32)

    def run(self, rate, stop=None, want=False, peak=False, momentum=None, init='own', seed=0):
        c = self.case
        return self.engine.synthesize(self.ids, c['S'], E.REF_DB, E.MAX_DB, E.POWER, c['n_iter'], c['win'], c['hop'],
                                      init_phase=self.init(rate) if isinstance(init, str) else init, seed=seed, peak_normalize=peak,
                                      want_mel=want, want_linear=want, want_alignments=want, momentum=momentum, stop_at_silence=stop,
                                      speaking_rate=rate)

    def reference(self, b, rate, n_in, n_out, momentum=0.0):
        """the Griffin-Lim oracle on the stretch oracle's blend of the oracle-de-normalised `linear` of utterance b: its first
        n_in frames stretched, zero frames up to n_out where the minimum length asks for them"""
        k = (b, rate, n_in, n_out, momentum)
        if k not in self._ref:
            c = self.case
            st = S.blend_f64(self.mag[b][:, :n_in], rate)
            mag = np.zeros((self.F, n_out))
            m = min(n_out, st.shape[1])
            mag[:, :m] = st[:, :m]
            init = self.init(rate)[b][:, :n_out]
            if momentum:
                self._ref[k] = M.griffin_lim_momentum(mag, c['win'], c['hop'], c['n_fft'], c['n_iter'], init, momentum=momentum)[0]
            else:
                self._ref[k] = A.griffin_lim_v2(mag, c['win'], c['hop'], c['n_fft'], c['n_iter'], init_phase=init)[0]
        return self._ref[k]

    def check(self, wav, rate, n_in, n_out, label, momentum=0.0):
        assert wav.shape == (self.case['B'], self.hop * (self.Tg(rate) - 1)), label
        for b in range(self.case['B']):
            m = self.hop * (int(n_out[b]) - 1)
            assert_segment_parity(wav[b, :m], self.reference(b, rate, int(n_in[b]), int(n_out[b]), momentum), self.hop,
                                  C.gl_tol(self.case['n_iter']), '{} b={} n={}->{}'.format(label, b, n_in[b], n_out[b]))
            assert not wav[b, m:].any() and not np.signbit(wav[b, m:]).any(), '{} b={}: the row tail is not 0.0'.format(label, b)

    def full(self):
        return [self.T] * self.case['B']


@pytest.fixture(scope='module')
def ref_case():
    c = Case(E.E2E)
    yield c
    c.engine.close()


@pytest.fixture(scope='module')
def small_case():
    c = Case(E.E2E_512)
    yield c
    c.engine.close()


@pytest.mark.parametrize('rate', RATES)
@pytest.mark.parametrize('which', ['streaming', 'general'])
def test_waveform_is_the_oracle_of_the_stretched_magnitudes(ref_case, small_case, which, rate):
    c = ref_case if which == 'streaming' else small_case
    Tg = c.Tg(rate)
    assert (c.T, rate, Tg) in [(40, 1.25, 32), (40, 0.8, 50), (25, 1.25, 20), (25, 0.8, 32)]
    out = c.run(rate, want=True)      # (the first call at a new rate: its buffers grow, it is not pipelined)
    wav = out['wav'].to_host()
    c.check(wav, rate, c.full(), [Tg] * c.case['B'], '{} rate {}'.format(which, rate))
    assert 'n_frames' not in out and c.engine.synth_frames(c.case['B']).tolist() == [Tg] * c.case['B']
    # nothing else of the call moves: the optional outputs keep their length T and the bits of the rate-1.0 call
    for k in ('mel', 'alignments', 'linear'):
        assert np.array_equal(bits(out[k].to_host()), bits(c.off[k])), k
    # ... and the same call again goes through the pipeline's streams (the initial phases on the front stream): the same bits
    again = c.run(rate)
    assert np.array_equal(bits(again['wav'].to_host()), bits(wav))
    c.engine.set_option('pipeline', 0)
    try:
        assert np.array_equal(bits(c.run(rate)['wav'].to_host()), bits(wav))
    finally:
        c.engine.set_option('pipeline', 1)
    assert c.engine._speaking_rate == 1.0     # the scope put the handle's setting back


@pytest.mark.parametrize('rate', RATES)
@pytest.mark.parametrize('which', ['streaming', 'general'])
def test_with_end_of_speech_stopping(ref_case, small_case, which, rate):
    c = ref_case if which == 'streaming' else small_case
    d = E.distance_from_threshold(c.linear, c.threshold_db)
    assert d >= E.OFF_THRESHOLD and len(set(c.lengths.tolist())) == c.case['B']
    Tg, minf = c.Tg(rate), c.case['min_frames']
    want = S.stretched_lengths(c.lengths, rate, Tg, minf)
    assert want.tolist() == [min(Tg, max(minf, int(np.ceil(n / rate)))) for n in c.lengths.tolist()]
    stop = (c.threshold_db, 0)
    out = c.run(rate, stop=stop, want=True)
    print('{} rate {}: oracle lengths {} -> {}, device {}'.format(which, rate, c.lengths, want, out['n_frames']))
    assert out['n_frames'].dtype == np.int32 and out['n_frames'].tolist() == want.tolist()
    wav = out['wav'].to_host()
    c.check(wav, rate, c.lengths, want, '{} eos rate {}'.format(which, rate))
    for k in ('mel', 'alignments', 'linear'):
        assert np.array_equal(bits(out[k].to_host()), bits(c.off[k])), k
    # per-utterance peak normalisation: tts_peak_normalize on the padded rows
    peak = c.run(rate, stop=stop, peak=True)
    assert peak['n_frames'].tolist() == want.tolist()
    assert np.array_equal(bits(peak['wav'].to_host()), bits(c.engine.peak_normalize(out['wav']).to_host()))
    # pipelined (this shape and setting have run) and not: the same bits and lengths
    c.engine.set_option('pipeline', 0)
    try:
        serial = c.run(rate, stop=stop)
    finally:
        c.engine.set_option('pipeline', 1)
    assert serial['n_frames'].tolist() == want.tolist() and np.array_equal(bits(serial['wav'].to_host()), bits(wav))


def test_utterances_shorter_than_griffin_lim_takes_are_padded_with_zero_frames(ref_case):
    """a threshold above every value: every utterance has min_frames = 5 frames, ceil(5 / 1.25) = 4 < 5 -- the fifth frame is
    the vocoder's zero padding; at rate 0.8 they get ceil(5 / 0.8) = 7"""
    c = ref_case
    B, minf = c.case['B'], c.case['min_frames']
    stop = (E.REF_DB + 1.0, 0)
    for rate, n_out in [(1.25, 5), (0.8, 7)]:
        assert S.stretched_frames(minf, 1.25) < minf
        out = c.run(rate, stop=stop)
        assert out['n_frames'].tolist() == [n_out] * B == S.stretched_lengths([minf] * B, rate, c.Tg(rate), minf).tolist()
        c.check(out['wav'].to_host(), rate, [minf] * B, [n_out] * B, 'all min_frames rate {}'.format(rate))
    # a threshold below every value: all T frames, all T' after the stretch -- the uniform call's bits
    low = c.run(1.25, stop=(-101.0, 0))
    assert low['n_frames'].tolist() == [c.Tg(1.25)] * B
    assert np.array_equal(bits(low['wav'].to_host()), bits(c.run(1.25)['wav'].to_host()))


def test_off_is_the_call_as_it_was(ref_case):
    """rate 1.0 -- never set, set explicitly, or set to something else and back -- gives the bits of the handle that never heard
    of the setting, and enqueues no stretch launch"""
    c = ref_case
    eng = c.engine
    H = pkg('_hip')
    want = c.off['wav']       # (made on the fresh handle, before any rate was set)
    c.run(1.25)
    assert eng._speaking_rate == 1.0
    assert np.array_equal(bits(c.run(None)['wav'].to_host()), bits(want))
    eng.set_speaking_rate(1.25)
    try:
        got = c.run(None, init=c.init(1.25))     # the handle's setting, read when the call is made
        assert got['wav'].shape == (c.case['B'], c.hop * (c.Tg(1.25) - 1))
        assert np.array_equal(bits(got['wav'].to_host()), bits(c.run(1.25)['wav'].to_host()))
    finally:
        eng.set_speaking_rate(1.0)
    eng.set_option('profile', 1)
    try:
        eng.profile_reset()
        assert np.array_equal(bits(c.run(1.0)['wav'].to_host()), bits(want))
        assert eng.profile_get('stretch') == (0.0, 0)
        c.run(1.25)
        assert eng.profile_get('stretch')[1] == 1
    finally:
        eng.set_option('profile', 0)
    # refused settings leave the handle's as it was
    for bad in (float('nan'), float('inf'), 0.0, 0.2, 4.5):
        assert eng.lib.tts_set_speaking_rate(eng.handle, bad) == H.TTS_ERR_INVALID
    assert eng.lib.tts_set_speaking_rate(None, 1.0) == H.TTS_ERR_INVALID
    assert np.array_equal(bits(c.run(None)['wav'].to_host()), bits(want))
    with pytest.raises(ValueError):
        c.run(1.25, init=c.init1)        # an init_phase of T frames for a call that reconstructs from T'


def test_a_rate_that_leaves_too_few_frames_is_refused(ref_case):
    """min_frames is 5 at 1102 / 275: three decoder steps at rate 4 leave ceil(15 / 4) = 4 frames, four leave exactly 5"""
    H = pkg('_hip')
    c, cs = ref_case, ref_case.case
    with pytest.raises(H.TtsError) as e:
        c.engine.synthesize(c.ids, 3, E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'], seed=1, peak_normalize=False,
                            speaking_rate=4.0)
    assert e.value.code == H.TTS_ERR_INVALID and 'speaking rate' in str(e.value)
    out = c.engine.synthesize(c.ids, 4, E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'], seed=1, peak_normalize=False,
                              speaking_rate=4.0)
    assert out['wav'].shape == (cs['B'], cs['hop'] * 4) and np.isfinite(out['wav'].to_host()).all()


def test_host_calls_return_the_same_bits_and_lengths(ref_case):
    """tts_synthesize_host at rate 1.25, three calls in flight, with and without end-of-speech stopping: the pinned buffers are
    sized for T', the bits and the lengths are tts_synthesize's"""
    c, cs = ref_case, ref_case.case
    eng = c.engine
    args = (cs['S'], E.REF_DB, E.MAX_DB, E.POWER, cs['n_iter'], cs['win'], cs['hop'])
    stop = (c.threshold_db, 0)
    Tg = c.Tg(1.25)
    want_plain = c.run(1.25, init=None, seed=9)['wav'].to_host()
    want_stop = c.run(1.25, stop=stop, init=None, seed=9)
    want_stop_wav, want_n = want_stop['wav'].to_host(), want_stop['n_frames']
    assert want_n.tolist() == S.stretched_lengths(c.lengths, 1.25, Tg, cs['min_frames']).tolist()
    t0 = eng.synthesize_host(E.ids_of(cs, seed=5), *args, seed=9, peak_normalize=False, speaking_rate=1.25)
    t1 = eng.synthesize_host(c.ids, *args, seed=9, peak_normalize=False, speaking_rate=1.25)
    t2 = eng.synthesize_host(c.ids, *args, seed=9, peak_normalize=False, speaking_rate=1.25, stop_at_silence=stop)
    assert eng.wait_host(t0).shape == (cs['B'], c.hop * (Tg - 1))
    assert eng.wait_host_frames(t1).tolist() == [Tg] * cs['B']
    got = eng.wait_host(t1)
    assert got.shape == want_plain.shape and np.array_equal(bits(got), bits(want_plain))
    assert eng.wait_host_frames(t2).tolist() == want_n.tolist()
    assert np.array_equal(bits(eng.wait_host(t2)), bits(want_stop_wav))
    off = eng.synthesize_host(c.ids, *args, seed=9, peak_normalize=False)
    assert eng.wait_host_frames(off).tolist() == c.full()
    assert np.array_equal(bits(eng.wait_host(off)), bits(c.run(None, init=None, seed=9)['wav'].to_host()))


def test_momentum_composes(ref_case):
    """gl_momentum = 990 with rate 1.25: the momentum oracle on the stretched magnitudes, at the bar the momentum tests use"""
    c = ref_case
    Tg = c.Tg(1.25)
    out = c.run(1.25, momentum=0.99)
    assert c.engine._gl_momentum == 0
    wav = out['wav'].to_host()
    c.check(wav, 1.25, c.full(), [Tg] * c.case['B'], 'rate 1.25 momentum', momentum=0.99)
    assert not np.array_equal(wav, c.run(1.25)['wav'].to_host())


def test_serve_post_processing_stretches_with_the_stage_calls(ref_case, monkeypatch):
    """tacotron.serve.post_process_spectrograms(speaking_rate=...): tts_denorm_power, tts_stretch_magnitudes and the (ragged)
    Griffin-Lim stage give the lengths and, to the Griffin-Lim bar, the waveforms of the call pipeline"""
    V = pkg('tacotron.serve')
    P = pkg('tacotron.params')
    c = ref_case
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', c.case['n_iter'])
    want = S.stretched_lengths(c.lengths, 1.25, c.Tg(1.25), c.case['min_frames'])
    wavs = V.post_process_spectrograms(c.linear, c.engine, init_phase=c.init(1.25), stop_at_silence_db=float(c.threshold_db),
                                       silence_keep_ms=0.0, speaking_rate=1.25)
    assert [len(w) for w in wavs] == [c.hop * (int(n) - 1) for n in want]
    piped = c.run(1.25, stop=(c.threshold_db, 0))['wav'].to_host()
    for b, w in enumerate(wavs):
        assert_segment_parity(w, piped[b, :len(w)], c.hop, C.gl_tol(c.case['n_iter']), 'serve b={}'.format(b))
    plain = V.post_process_spectrograms(c.linear, c.engine, init_phase=c.init(0.8), speaking_rate=0.8)
    assert [len(w) for w in plain] == [c.hop * (c.Tg(0.8) - 1)] * c.case['B']


# ---------------------------------------------------------------------------------------------- the waveform effect
@pytest.mark.parametrize('rate', [0.8, 1.25])
def test_engine_time_stretch(engine, rate):
    """one 4096-sample waveform: |STFT| (n_fft 1024, window 1024, hop 256) to the analysis bar, the exact blend of the device's
    own magnitudes, and a waveform of 256 (T' - 1) samples"""
    y = C.tone_noise(np.random.default_rng(4), 4096)
    T = 1 + 4096 // 256
    Tg = S.stretched_frames(T, rate)
    assert (T, Tg) == (17, {0.8: 22, 1.25: 14}[rate])
    wav, mag, st = engine.time_stretch(y, rate, n_iter=3, seed=5, want_magnitudes=True)
    mag_h, st_h, wav_h = mag.to_host(), st.to_host(), wav.to_host()
    ref = np.abs(A.stft(y, 1024, 256, 1024, dtype=np.complex128))
    assert mag_h.shape == (1, 513, T)
    assert_parity(mag_h, ref[None], C.STFT_AXES, C.ANALYSIS_TOL, 'time_stretch |stft|')
    assert np.array_equal(bits(st_h), bits(S.blend_batch(mag_h, rate)))
    assert wav_h.shape == (256 * (Tg - 1),) and np.isfinite(wav_h).all() and np.abs(wav_h).max() > 0
    # ... and a uniform batch of two
    both = engine.time_stretch(np.stack([y, y[::-1].copy()]), rate, n_iter=3, seed=5)
    assert both.shape == (2, 256 * (Tg - 1))
    for a in (wav, mag, st, both):
        a.free()
