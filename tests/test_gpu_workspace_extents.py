"""GPU: no workspace of a synthesis call grows in a pipelined call.  A buffer that grows makes the library synchronise every
stream of the handle -- the wait the call pipeline is built to avoid -- so every workspace of a call is sized before anything of
it is enqueued, from the one function that declares the stage's buffers, which the stage itself asks again.  Here every setting is
on from the first call; after four identical calls every one of those buffers is where it was after the first, as large as it
was, and the calls' waveforms have the same bits.

Shapes: the two small end-to-end cases of eos_cases.py (streaming kernel, B = 3, 40 frames of 275 samples; general kernels at
n_fft 512, 25 frames of 100) -- the smallest at which every stage of a call runs -- at the power and sampling rate the loudness
and limiter tests run them at."""
import numpy as np
import pytest

import eos_cases as E
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED = 9
SR = 8000
POWER = 0.3
SETTINGS = dict(momentum=0.5, phase_init='estimate', speaking_rate=0.8, pitch=4.0 / 12.0, loudness=(-23.0, 1e6),
                limiter=(0.05, 2.0, 4), alignment_stats=True)
COMMON = ['lim.out', 'lim.flags', 'lim.stats', 'loud.ws', 'loud.z', 'loud.peak', 'pe.u_rows', 'pe.mag_rows', 'pe.map_s', 'pe.map_o',
          'pe.start', 'gl.init_est', 'gl.rag_rw', 'gl.rag_lens', 'eos.active', 'eos.frames', 'gl.mag', 'gl.mag_st', 'gl.wav_pitch',
          'syn.phase0.even', 'syn.phase1.even', 'syn.phase0.odd', 'syn.phase1.odd']
BY_FAMILY = {True: ['gl.mom', 'gl.mse_partial', 'gl.counter_ring'], False: ['glg.phase', 'glg.frames', 'glg.mse_partial', 'glg.mom']}
# what every case must have (the rest exists or not by the case: a chunk map only with more than one chunk of frames, ...)
ALWAYS = ['lim.out', 'loud.ws', 'pe.u_rows', 'gl.init_est', 'gl.rag_rw', 'gl.rag_lens', 'eos.active', 'eos.frames', 'gl.mag', 'gl.mag_st',
          'gl.wav_pitch', 'syn.phase0.even', 'syn.phase0.odd']


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine_of(case):
    eng = pkg().Engine(E.hparams_of(case))   # (the library's own stream: the call pipeline is on)
    eng.sampling_rate = SR
    eng.load_weights(E.weights_of(case))
    return eng


def extents(eng, names):
    H = pkg('_hip')
    out = {}
    for name in names:
        try:
            out[name] = eng.debug_workspace_extent(name)
        except H.TtsError:
            pass                                  # (no such buffer in this case)
    return out


@pytest.mark.parametrize('name', ['E2E', 'E2E_512'])
def test_no_workspace_moves_or_grows_after_the_first_call(name):
    case = getattr(E, name)
    args = (E.ids_of(case), case['S'], E.REF_DB, E.MAX_DB, POWER, case['n_iter'], case['win'], case['hop'])
    scout = engine_of(case)                       # the threshold, from the linear spectrograms of a call on another handle
    try:
        threshold_db = E.choose_threshold(scout.synthesize(*args, seed=SEED, want_linear=True)['linear'].to_host(), case['min_frames'])
    finally:
        scout.close()
    assert threshold_db is not None
    streaming = case['n_fft'] == 2048
    names = COMMON + BY_FAMILY[streaming]
    eng = engine_of(case)
    try:
        wavs, first = [], None
        for _ in range(4):
            out = eng.synthesize(*args, seed=SEED, peak_normalize=True, stop_at_silence=(threshold_db, 0), **SETTINGS)
            wavs.append(out['wav'])
            if first is None:
                first = extents(eng, names)
                lengths = out['n_frames'].tolist()
        eng.synchronize()
        last = extents(eng, names)
        host = [w.to_host() for w in wavs]
    finally:
        eng.close()
    print(name, 'lengths', lengths)
    for k in sorted(set(first) | set(last)):
        print('  {:18s} first {}  last {}'.format(k, first.get(k), last.get(k)))
    assert len(set(lengths)) == case['B']                                 # a ragged call
    assert set(ALWAYS + BY_FAMILY[streaming]) <= set(first), sorted(set(ALWAYS + BY_FAMILY[streaming]) - set(first))
    assert last == first
    for w in host[1:]:
        assert np.array_equal(bits(w), bits(host[0]))
