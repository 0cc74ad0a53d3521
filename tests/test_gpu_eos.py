"""GPU: end-of-speech stopping -- tts_speech_frames against the oracle (tests/eos_oracle.py, a restatement of the
reference's silence_interval_from_spectrogram, audio/effects.py:218-233) by exact integer equality, and the feature inside
tts_synthesize / tts_synthesize_host: the lengths are the oracle's, every utterance is the Griffin-Lim oracle's
reconstruction of its own frames, the rest of its row is 0 and nothing else of the call moves.

The end-to-end cases (eos_cases.py) are the smallest that reach every path: B = 3, T = 40 at the reference architecture
(streaming kernel; the shortest legal utterance has 5 frames) and T = 25 at n_fft = 512 (general kernels; 4 frames).  The
threshold is chosen from the device's own `linear` in the middle of a gap between the frames' maxima so that the three
lengths differ, and the test asserts that every maximum is at least 1e-3 normalised units away from it."""
import ctypes
import math

import numpy as np
import pytest

import audio_cases as C
import eos_cases as K
import eos_oracle as E
import momentum_oracle as M
from conftest import pkg
from oracle import audio_oracle as A
from parity import assert_segment_parity

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- tts_speech_frames
def _frames(engine, spec, thr, keep=0, minf=1, row_stride=None):
    n, last = engine.speech_frames(spec, thr, keep_frames=keep, min_frames=minf, row_stride=row_stride)
    out = n.to_host(), last.to_host()
    n.free()
    last.free()
    return out


@pytest.mark.parametrize('pad,fill', [(0, 0.0), (3, np.nan), (3, np.inf)], ids=['dense', 'pad-nan', 'pad-inf'])
@pytest.mark.parametrize('F', K.STAGE_F)
def test_speech_frames_equals_the_oracle(engine, F, pad, fill):
    x = K.stage_batch(F)
    full, view = K.padded(x, pad, fill) if pad else (x, x)
    stride = F + pad if pad else None
    for keep in (0, 3, 100):
        for minf in (1, 5, K.STAGE_T):
            want_n, want_last = E.speech_frames_batch(x, K.STAGE_THRESHOLD, keep, minf)
            n, last = _frames(engine, view, K.STAGE_THRESHOLD, keep, minf, stride)
            assert last.tolist() == want_last.tolist() == K.STAGE_EXPECT_LAST, (F, pad, keep, minf)
            assert n.tolist() == want_n.tolist(), (F, pad, keep, minf)


@pytest.mark.parametrize('F', [1025, 1])
def test_speech_frames_does_not_depend_on_the_batch(engine, F):
    """an utterance alone, and the batch in another order (rows of 1025 floats then start at other alignments)"""
    x = K.stage_batch(F)
    n, last = _frames(engine, x, K.STAGE_THRESHOLD, 2, 3)
    rn, rlast = _frames(engine, np.ascontiguousarray(x[::-1]), K.STAGE_THRESHOLD, 2, 3)
    assert rn.tolist() == n[::-1].tolist() and rlast.tolist() == last[::-1].tolist()
    for b in range(len(x)):
        one_n, one_last = _frames(engine, x[b:b + 1], K.STAGE_THRESHOLD, 2, 3)
        assert (one_n[0], one_last[0]) == (n[b], last[b])


def test_speech_frames_one_frame_one_bin(engine):
    for value, want in [(0.6, (1, 0)), (0.5, (1, -1)), (np.nan, (1, -1)), (np.inf, (1, 0)), (-np.inf, (1, -1))]:
        n, last = _frames(engine, np.full((1, 1, 1), value, np.float32), np.float32(0.5), keep=7)
        assert (n[0], last[0]) == want, value
    n, last = _frames(engine, np.full((1, 1, 1), -np.inf, np.float32), -np.inf)   # -Inf > -Inf is False
    assert (n[0], last[0]) == (1, -1)


def test_speech_frames_refusals_leave_the_outputs_untouched(engine):
    H = pkg('_hip')
    B, T, F = 2, 6, 8
    spec = engine.to_device(np.ones((B, T, F), np.float32))
    n = engine.to_device(np.full(B, -7, np.int32))
    last = engine.to_device(np.full(B, -9, np.int32))
    call = lambda *a: engine.lib.tts_speech_frames(engine.handle, *a)   # noqa: E731
    sp, pn, pl = spec.data_ptr(), n.data_ptr(), last.data_ptr()
    nan = float('nan')
    try:
        bad = [(sp, 0, T, F, F, 0.5, 0, 1, pn, pl), (sp, B, 0, F, F, 0.5, 0, 1, pn, pl), (sp, B, T, 0, F, 0.5, 0, 1, pn, pl),
               (sp, B, T, F, F - 1, 0.5, 0, 1, pn, pl), (sp, B, T, F, F, 0.5, -1, 1, pn, pl), (sp, B, T, F, F, 0.5, 0, 0, pn, pl),
               (sp, B, T, F, F, 0.5, 0, T + 1, pn, pl), (sp, B, T, F, F, nan, 0, 1, pn, pl), (None, B, T, F, F, 0.5, 0, 1, pn, pl),
               (sp, B, T, F, F, 0.5, 0, 1, None, pl)]
        for args in bad:
            assert call(*args) == H.TTS_ERR_INVALID, args
        engine.synchronize()
        assert n.to_host().tolist() == [-7] * B and last.to_host().tolist() == [-9] * B
        assert call(sp, B, T, F, F, 0.5, 0, 1, pn, None) == H.TTS_OK    # last_active may be NULL
        assert n.to_host().tolist() == [T] * B and last.to_host().tolist() == [-9] * B
        with pytest.raises(ValueError):
            engine.speech_frames(np.ones((T, F), np.float32), 0.5)
    finally:
        for a in (spec, n, last):
            a.free()


def test_speech_frames_profile_stage_and_python_threshold(engine):
    x = K.stage_batch(129)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        _frames(engine, x, K.STAGE_THRESHOLD)
        ms, launches = engine.profile_get('speech_end')
    finally:
        engine.set_option('profile', 0)
    assert launches == 2 and ms > 0
    ref, mx = float(np.float32(K.REF_DB)), float(np.float32(K.MAX_DB))
    assert engine.speech_threshold(-40.0, K.REF_DB, K.MAX_DB) == np.float32((-40.0 - ref) / (abs(ref) + abs(mx)) + 1.0)
    assert engine.speech_threshold(-40.0, K.REF_DB, K.MAX_DB, power=K.POWER) == np.float32(
        math.pow(math.pow(10.0, -40.0 / 20.0), float(np.float32(K.POWER))))
    with pytest.raises(ValueError):
        engine.speech_threshold(float('nan'), K.REF_DB, K.MAX_DB)


# ---------------------------------------------------------------------------------------------- end to end
class Case(object):
    """an engine of the case's architecture, the feature-off call (made once) and what the tests derive from it"""

    def __init__(self, case):
        self.case = case
        self.hp = K.hparams_of(case)
        self.engine = pkg().Engine(self.hp)
        self.engine.load_weights(K.weights_of(case))
        self.ids = K.ids_of(case)
        self.init = K.init_of(case)
        self.T = case['S'] * self.hp.reduction
        self.hop = case['hop']
        off = self.run(want=True)
        self.off = {k: off[k].to_host() for k in ('wav', 'mel', 'linear')}
        assert 'n_frames' not in off and self.engine.synth_frames(case['B']).tolist() == [self.T] * case['B']
        self.linear = self.off['linear']
        self.threshold_db = K.choose_threshold(self.linear, case['min_frames'])
        assert self.threshold_db is not None, 'no gap between the frame maxima gives three different lengths'
        self.lengths = K.oracle_lengths(self.linear, self.threshold_db, 0, case['min_frames'])
        self._ref = {}

    def run(self, stop=None, want=False, peak=False, momentum=None, ids=None, init='own', seed=0):
        c = self.case
        return self.engine.synthesize(self.ids if ids is None else ids, c['S'], K.REF_DB, K.MAX_DB, K.POWER, c['n_iter'], c['win'], c['hop'],
                                      init_phase=self.init if isinstance(init, str) else init, seed=seed, peak_normalize=peak, want_mel=want,
                                      want_linear=want, momentum=momentum, stop_at_silence=stop)

    def stop(self, keep=0):
        return (self.threshold_db, keep)

    def reference(self, b, n, momentum=0.0):
        """the Griffin-Lim oracle on the oracle-de-normalised `linear` of utterance b cut to n columns, same phases cut the same way"""
        k = (b, n, momentum)
        if k not in self._ref:
            c = self.case
            mag = A.linear_to_magnitude(self.linear[b], K.REF_DB, K.MAX_DB, K.POWER)[:, :n]
            if momentum:
                self._ref[k] = M.griffin_lim_momentum(mag, c['win'], c['hop'], c['n_fft'], c['n_iter'], self.init[b][:, :n], momentum=momentum)[0]
            else:
                self._ref[k] = A.griffin_lim_v2(mag, c['win'], c['hop'], c['n_fft'], c['n_iter'], init_phase=self.init[b][:, :n])[0]
        return self._ref[k]

    def check(self, wav, lengths, label, momentum=0.0):
        assert wav.shape == (self.case['B'], self.hop * (self.T - 1))
        for b, n in enumerate(lengths):
            m = self.hop * (int(n) - 1)
            assert_segment_parity(wav[b, :m], self.reference(b, int(n), momentum), self.hop, C.gl_tol(self.case['n_iter']),
                                  '{} b={} n={}'.format(label, b, n))
            assert not wav[b, m:].any() and not np.signbit(wav[b, m:]).any(), '{} b={}: the row tail is not 0.0'.format(label, b)


@pytest.fixture(scope='module')
def ref_case():
    c = Case(K.E2E)
    yield c
    c.engine.close()


@pytest.fixture(scope='module')
def small_case():
    c = Case(K.E2E_512)
    yield c
    c.engine.close()


def test_the_input_stays_off_the_threshold(ref_case, small_case):
    for c in (ref_case, small_case):
        d = K.distance_from_threshold(c.linear, c.threshold_db)
        print('n_fft {}: threshold {} dB, oracle lengths {}, distance {:.3e}'.format(c.case['n_fft'], c.threshold_db, c.lengths, d))
        assert d >= K.OFF_THRESHOLD
        assert len(set(c.lengths.tolist())) == c.case['B']


def test_lengths_and_waveforms_are_the_oracles(ref_case):
    c = ref_case
    out = c.run(stop=c.stop(), want=True)
    print('lengths {} oracle {}'.format(out['n_frames'], c.lengths))
    assert out['n_frames'].dtype == np.int32 and out['n_frames'].tolist() == c.lengths.tolist()
    c.check(out['wav'].to_host(), c.lengths, 'eos 2048')
    # nothing else of the call moves: the optional outputs stay full length, bit for bit
    assert np.array_equal(bits(out['linear'].to_host()), bits(c.off['linear']))
    assert np.array_equal(bits(out['mel'].to_host()), bits(c.off['mel']))
    # keep_frames reaches the lengths as the oracle's clamp says
    kept = c.run(stop=c.stop(keep=4))
    want = K.oracle_lengths(c.linear, c.threshold_db, 4, c.case['min_frames'])
    assert kept['n_frames'].tolist() == want.tolist() and want.tolist() != c.lengths.tolist()
    c.check(kept['wav'].to_host(), want, 'eos 2048 keep 4')


def test_general_kernels(small_case):
    c = small_case
    assert c.case['min_frames'] == 4
    out = c.run(stop=c.stop(), want=True)
    assert out['n_frames'].tolist() == c.lengths.tolist()
    c.check(out['wav'].to_host(), c.lengths, 'eos 512')
    assert np.array_equal(bits(out['linear'].to_host()), bits(c.off['linear']))
    assert np.array_equal(bits(out['mel'].to_host()), bits(c.off['mel']))
    peak = c.run(stop=c.stop(), peak=True)
    assert np.array_equal(bits(peak['wav'].to_host()), bits(c.engine.peak_normalize(out['wav']).to_host()))


def test_pipelined_unpipelined_and_third_of_three(ref_case):
    c = ref_case
    eng = c.engine
    pipelined = c.run(stop=c.stop())   # (the engine has run this shape: the call goes through the pipeline's streams)
    want_wav, want_n = pipelined['wav'].to_host(), pipelined['n_frames']
    assert want_n.tolist() == c.lengths.tolist()
    eng.set_option('pipeline', 0)
    try:
        serial = c.run(stop=c.stop())
    finally:
        eng.set_option('pipeline', 1)
    assert serial['n_frames'].tolist() == want_n.tolist() and np.array_equal(bits(serial['wav'].to_host()), bits(want_wav))
    # three calls back to back on device-resident inputs, other sentences in front
    dev_ids = [eng.to_device(K.ids_of(c.case, seed=s)) for s in (5, 6)] + [eng.to_device(c.ids)]
    dev_init = eng.to_device(c.init)
    outs = [c.run(stop=c.stop(), ids=d, init=dev_init) for d in dev_ids]
    eng.synchronize()
    assert outs[2]['n_frames'].tolist() == want_n.tolist()
    assert np.array_equal(bits(outs[2]['wav'].to_host()), bits(want_wav))
    for o in outs[:2]:   # (other sentences: other spectrograms, lengths within the call's range)
        assert all(c.case['min_frames'] <= v <= c.T for v in o['n_frames'].tolist())


def test_host_calls_return_the_same_bits_and_lengths(ref_case):
    """tts_synthesize_host + tts_wait_host_frames, three calls in flight: the phases are drawn from the seed"""
    c, cs = ref_case, ref_case.case
    eng = c.engine
    args = (cs['S'], K.REF_DB, K.MAX_DB, K.POWER, cs['n_iter'], cs['win'], cs['hop'])
    want = c.run(stop=c.stop(), init=None, seed=9)
    want_wav, want_n = want['wav'].to_host(), want['n_frames']
    tickets = [eng.synthesize_host(K.ids_of(cs, seed=s), *args, seed=9, peak_normalize=False, stop_at_silence=c.stop()) for s in (5, 6)]
    tickets.append(eng.synthesize_host(c.ids, *args, seed=9, peak_normalize=False, stop_at_silence=c.stop()))
    off = eng.synthesize_host(c.ids, *args, seed=9, peak_normalize=False)   # (the set of the first ticket is reused: wait for it first)
    got_n = [None, None, eng.wait_host_frames(tickets[2])]
    got = eng.wait_host(tickets[2])
    assert got_n[2].dtype == np.int32 and got_n[2].tolist() == want_n.tolist()
    assert np.array_equal(bits(got), bits(want_wav))
    assert eng.wait_host_frames(off).tolist() == [c.T] * cs['B']
    assert np.array_equal(bits(eng.wait_host(off)), bits(c.run(init=None, seed=9)['wav'].to_host()))


def test_peak_normalised_is_peak_normalize_of_the_plain_result(ref_case):
    c = ref_case
    plain = c.run(stop=c.stop())
    peak = c.run(stop=c.stop(), peak=True)
    assert peak['n_frames'].tolist() == c.lengths.tolist()
    got = peak['wav'].to_host()
    want = c.engine.peak_normalize(plain['wav']).to_host()
    assert np.array_equal(bits(got), bits(want))
    for b, n in enumerate(c.lengths):
        m = c.hop * (int(n) - 1)
        assert abs(np.abs(got[b, :m]).max() - 1.0) < 1e-6 and not got[b, m:].any()


def test_thresholds_below_and_above_every_value(ref_case):
    c = ref_case
    low = c.run(stop=(-101.0, 0))
    assert low['n_frames'].tolist() == [c.T] * c.case['B']
    assert np.array_equal(bits(low['wav'].to_host()), bits(c.off['wav']))
    high = c.run(stop=(K.REF_DB + 1.0, 0))
    assert high['n_frames'].tolist() == [c.case['min_frames']] * c.case['B']
    c.check(high['wav'].to_host(), high['n_frames'], 'eos 2048 all min_frames')
    # ... and with frames kept behind nothing: min(T, max(min_frames, 0 + keep))
    assert c.run(stop=(K.REF_DB + 1.0, 11))['n_frames'].tolist() == [11] * c.case['B']
    assert c.run(stop=(K.REF_DB + 1.0, 1000))['n_frames'].tolist() == [c.T] * c.case['B']


def test_the_setting_leaves_no_trace_and_scopes_to_the_call(ref_case):
    c = ref_case
    eng = c.engine
    c.run(stop=c.stop())
    assert eng._end_of_speech == (False, 0.0, 0)            # the scope put the handle's setting back
    eng.set_end_of_speech(True, c.threshold_db, 0)
    try:
        assert c.run()['n_frames'].tolist() == c.lengths.tolist()     # the handle's setting, read when the call is made
    finally:
        eng.set_end_of_speech(False)
    after = c.run()
    assert sorted(after) == ['alignments', 'linear', 'mel', 'wav'] and eng.synth_frames(c.case['B']).tolist() == [c.T] * c.case['B']
    fresh = Case.__new__(Case)
    fresh.case, fresh.hp, fresh.ids, fresh.init = c.case, c.hp, c.ids, c.init
    fresh.engine = pkg().Engine(c.hp)
    try:
        fresh.engine.load_weights(K.weights_of(c.case))
        want = fresh.run()['wav'].to_host()
    finally:
        fresh.engine.close()
    assert np.array_equal(bits(after['wav'].to_host()), bits(want))
    H = pkg('_hip')
    for bad in [(float('nan'), 0), (-40.0, -1)]:
        with pytest.raises(ValueError):
            c.run(stop=bad)
        assert eng.lib.tts_set_end_of_speech(eng.handle, 1, ctypes.c_float(bad[0]), bad[1]) == H.TTS_ERR_INVALID
    c.run()
    assert eng.synth_frames(c.case['B']).tolist() == [c.T] * c.case['B']       # a refused setting changes nothing
    with pytest.raises(H.TtsError):
        eng.synth_frames(c.case['B'] + 1)


def test_momentum_with_the_feature_on(ref_case):
    """alpha = 0.99: the lengths do not depend on it, the waveforms stay within the bound the ragged momentum test uses"""
    c = ref_case
    out = c.run(stop=c.stop(), momentum=0.99)
    assert out['n_frames'].tolist() == c.lengths.tolist()
    c.check(out['wav'].to_host(), c.lengths, 'eos 2048 momentum', momentum=0.99)
    assert not np.array_equal(out['wav'].to_host(), c.run(stop=c.stop())['wav'].to_host())


def test_a_call_too_short_for_the_feature_is_refused(ref_case):
    """hop 100 at n_fft 2048 (general kernels): min_frames is 12, one decoder step gives T = 5"""
    H = pkg('_hip')
    c, cs = ref_case, ref_case.case
    with pytest.raises(H.TtsError) as e:
        c.engine.synthesize(c.ids, 1, K.REF_DB, K.MAX_DB, K.POWER, cs['n_iter'], 400, 100, seed=1, peak_normalize=False,
                            stop_at_silence=c.stop())
    assert e.value.code == H.TTS_ERR_INVALID and 'end-of-speech' in str(e.value)
    assert c.run(stop=c.stop())['n_frames'].tolist() == c.lengths.tolist()


def test_command_line_writes_wavs_of_different_lengths(ref_case, tmp_path, monkeypatch):
    """python -m <package>.tacotron.inference --stop-at-silence DB --silence-keep-ms 0 (main() in this process): every file
    ends where the oracle says its utterance ends.  The threshold comes from the same sentences' `linear`, off every maximum."""
    I = pkg('tacotron.inference')   # noqa: E741
    P = pkg('tacotron.params')
    io = pkg('audio.io')
    sentences = ['The quick brown fox.', 'zzzzzzzzzz', 'No.']
    dataset = pkg('datasets.lj_speech').LJSpeechDatasetHelper(dataset_folder=P.dataset_params.dataset_folder,
                                                               char_dict=P.dataset_params.vocabulary_dict, fill_dict=False)
    seqs, lens = dataset.process_sentences(sentences)
    ids = np.array([I.pad_sentence(np.frombuffer(s, dtype=np.int32), max(lens)) for s in seqs], dtype=np.int32)
    S, min_frames = 8, 5
    loader = P.dataset_params.dataset_loader
    assert (loader.mel_mag_ref_db, loader.mel_mag_max_db, P.model_params.magnitude_power) == (K.REF_DB, K.MAX_DB, K.POWER)
    lin = ref_case.engine.synthesize(ids, S, K.REF_DB, K.MAX_DB, K.POWER, 2, 1102, 275, seed=0, peak_normalize=False,
                                     want_linear=True)['linear'].to_host()
    thr = K.choose_threshold(lin, min_frames)
    assert thr is not None and K.distance_from_threshold(lin, thr) >= K.OFF_THRESHOLD
    want = K.oracle_lengths(lin, thr, 0, min_frames)
    assert len(set(want.tolist())) == 3
    (tmp_path / 'sentences.txt').write_text('\n'.join(sentences) + '\n')
    out = tmp_path / 'out'
    out.mkdir()
    np.savez(tmp_path / 'weights.npz', **K.weights_of(K.E2E))
    monkeypatch.setattr(P.model_params.decoder, 'maximum_iterations', S * P.model_params.reduction)
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', 2)
    assert I.main(['--synthesis-file', str(tmp_path / 'sentences.txt'), '--synthesis-dir', str(out), '--weights',
                   str(tmp_path / 'weights.npz'), '--stop-at-silence', repr(float(thr)), '--silence-keep-ms', '0']) == 0
    got = []
    for i in range(3):
        wav, sr = io.load_wav(str(out / '{}.wav'.format(i + 1)))
        assert sr == 22050 and np.isfinite(wav).all() and abs(np.abs(wav).max() - 1.0) < 1e-6
        got.append(len(wav))
    print('wav lengths {} for {} frames'.format(got, want))
    assert got == [275 * (int(n) - 1) for n in want]


def test_serve_post_processing_cuts_in_normalised_units(ref_case, monkeypatch):
    """tacotron.serve.post_process_spectrograms(stop_at_silence_db=...): tts_speech_frames on the NORMALISED spectrograms
    (tts_speech_threshold's other units) gives the lengths the call pipeline finds on the magnitudes, and every waveform comes
    back at its own length"""
    V = pkg('tacotron.serve')
    P = pkg('tacotron.params')
    c = ref_case
    monkeypatch.setattr(P.model_params, 'reconstruction_iterations', c.case['n_iter'])
    wavs = V.post_process_spectrograms(c.linear, c.engine, init_phase=c.init, stop_at_silence_db=float(c.threshold_db), silence_keep_ms=0.0)
    assert [len(w) for w in wavs] == [c.hop * (int(n) - 1) for n in c.lengths]
    piped = c.run(stop=c.stop())['wav'].to_host()
    for b, w in enumerate(wavs):   # (the stages de-normalise with tts_denorm_power, the pipeline in the final Dense's epilogue)
        assert_segment_parity(w, piped[b, :len(w)], c.hop, C.gl_tol(c.case['n_iter']), 'serve b={}'.format(b))


@pytest.mark.parametrize('wide_from', [0, 1])
def test_the_wide_cut_of_a_ragged_batch_does_not_reach_the_bits(ref_case, wide_from):
    """Under the call pipeline a ragged batch is cut twice -- for the compute units beside the next call's decoder and, from
    launch `wide_from` on, for all of them (planned where that launch comes up).  At B = 3 the rule never picks a wide
    launch, so the option names it: 0 = every launch and the final iSTFT, 1 = the first launch narrow, the rest wide.  The
    call is pipelined (the engine has run this shape with the setting on; a persistent decoder covers it): the same lengths
    and the same bits as with the rule, peak normalisation included (its partials come from the wide cut's runs)."""
    c = ref_case
    eng = c.engine
    assert eng.decoder_kernel_choice(c.case['B'], c.case['Ts'], pipelined=True) != 0    # (else gl_wide_from gives no wide launch)
    def run(per_launch):
        eng.set_option('gl_pair', per_launch)
        try:
            out = c.run(stop=c.stop(), peak=True)
            return out['n_frames'].tolist(), out['wav'].to_host()
        finally:
            eng.set_option('gl_pair', 3)

    # three iterations: one launch, or three of one iteration (launches 1 and 2 then differ in their cut at wide_from = 1)
    want = {pl: run(pl) for pl in (3, 1)}
    eng.set_option('gl_wide_from', wide_from)
    try:
        got = {pl: run(pl) for pl in (3, 1)}
    finally:
        eng.set_option('gl_wide_from', -1)
    for pl in (3, 1):
        assert got[pl][0] == want[pl][0] == c.lengths.tolist()
        assert np.array_equal(bits(got[pl][1]), bits(want[pl][1])), pl
