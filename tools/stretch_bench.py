#!/usr/bin/env python3
"""The speaking rate (tts_set_speaking_rate) on an MI355X: the two stretch kernels alone at 64 x 1000 x 1025,
and whole calls at bench.py's shape -- 64 utterances x 150 ids, 200 decoder steps (1000 frames), 60 Griffin-Lim iterations,
seeded phases, peak normalisation, calls back to back on device-resident ids; ms per batch from a host clock around `--steps`
calls that end in one synchronise, after `--warmup` calls.

    python tools/stretch_bench.py [--steps 20] [--warmup 3] [--rounds 2] [--rates 1.25,0.8] [--skip-calls] [--skip-kernels]

Lines:
  (a) tts_stretch_rows (time-major rows of 1056 floats, the call pipeline's buffer) and tts_stretch_magnitudes ((F, T), the
      reference layout) at every rate: device time per call (profile stage "stretch") and achieved bytes per second --
      the input rows that are read once (min(T, T') rows: at a rate above 1 every output frame has its own two neighbours,
      below 1 neighbouring outputs share theirs) plus the output written -- as a fraction of tts_speech_frames' recorded
      read rate on the same buffer (5.5 TB/s, profiles/eos.txt: a yardstick only, for a pass that also writes);
  (b) whole calls at rate 1.0 and at every rate, alternating within a round: ms per batch and the stage times per batch.  The
      expectation: the Griffin-Lim stage scales with T' / T, and the call is bounded below by the next call's encoder and
      decoder, which always run all their steps (profiles/eos.txt found that for trimming)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--rounds', type=int, default=2)
ap.add_argument('--rates', default='1.25,0.8')
ap.add_argument('--skip-calls', action='store_true')
ap.add_argument('--skip-kernels', action='store_true')
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
P = importlib.import_module('single-speaker-tts_amd.tacotron.params')
W = importlib.import_module('single-speaker-tts_amd.tacotron.weights')
B, TS, N_STEPS, N_ITER = 64, 150, 200, 60
WIN, HOP, N_FFT = 1102, 275, 2048
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3
YARDSTICK = 5.5e12   # bytes per second: tts_speech_frames reading the same buffer (profiles/eos.txt)
rates = [float(r) for r in args.rates.split(',')]

hp = P.ModelParams()
eng = sstts.Engine(hp)
T, F, FP = N_STEPS * hp.reduction, 1 + N_FFT // 2, 1056

# ---- (a) the kernels alone
if not args.skip_kernels:
    rng = np.random.default_rng(0)
    rows_in = eng.empty((B, T, FP))
    cols_in = eng.empty((B, F, T))
    chunk = rng.random((T, FP)).astype(np.float32)
    for b in range(B):   # (filled utterance by utterance: 270 MB of host random numbers are not needed)
        eng._check(eng.lib.tts_memcpy_h2d(eng.handle, rows_in.ptr + b * chunk.nbytes, chunk.ctypes.data, chunk.nbytes))
        part = chunk[:, :F].T.copy()
        eng._check(eng.lib.tts_memcpy_h2d(eng.handle, cols_in.ptr + b * part.nbytes, part.ctypes.data, part.nbytes))
    eng.set_option('profile', 1)
    for rate in rates:
        T_out = eng.stretched_frames(T, rate)
        rows_out = eng.empty((B, T_out, FP))
        cols_out = eng.empty((B, F, T_out))
        nbytes = 4.0 * B * F * (min(T, T_out) + T_out)
        calls = {
            'tts_stretch_rows       [B][T][1056]': lambda: eng.lib.tts_stretch_rows(eng.handle, rows_in.ptr, B, T, F, FP, None, rate, T_out, rows_out.ptr),
            'tts_stretch_magnitudes [B][F][T]   ': lambda: eng.lib.tts_stretch_magnitudes(eng.handle, cols_in.ptr, B, F, T, None, rate, T_out, cols_out.ptr),
        }
        for name, call in calls.items():
            for rep in range(2):
                for _ in range(3):
                    eng._check(call())
                eng.profile_reset()
                for _ in range(20):
                    eng._check(call())
                ms, launches = eng.profile_get('stretch')
                ms /= 20
                rate_bps = nbytes / (ms * 1e-3)
                print('(a) {} rate {}: {} -> {} frames, {:.1f} us per call ({} launch), {:.0f} MB -> {:.2f} TB/s, {:.2f} of the {:.1f} TB/s '
                      'tts_speech_frames reads at'.format(name, rate, T, T_out, ms * 1e3, launches // 20, nbytes / 1e6, rate_bps / 1e12,
                                                          rate_bps / YARDSTICK, YARDSTICK / 1e12), flush=True)
        rows_out.free()
        cols_out.free()
    eng.set_option('profile', 0)
    rows_in.free()
    cols_in.free()

# ---- (b) whole calls
if not args.skip_calls:
    eng.load_weights(W.synthetic_weights(0, hp))
    rng = np.random.default_rng(1234)
    ids_h = rng.integers(2, hp.vocabulary_size, (B, TS)).astype(np.int32)
    ids_h[:, -1] = 1
    ids = eng.to_device(ids_h)
    wavs = {r: eng.empty((B, HOP * ((T if r == 1.0 else eng.stretched_frames(T, r)) - 1))) for r in [1.0] + rates}
    calls = [0]

    def timed(rate):
        def step():
            calls[0] += 1
            eng.synthesize(ids, N_STEPS, REF_DB, MAX_DB, POWER, N_ITER, WIN, HOP, seed=calls[0], peak_normalize=True, wav=wavs[rate],
                           speaking_rate=rate)
        for _ in range(args.warmup):
            step()
        eng.set_option('profile', 1)
        eng.profile_reset()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        stages = {s: eng.profile_get(s)[0] / args.steps for s in ('postnet', 'stretch', 'gl_iter', 'gl_final')}
        eng.set_option('profile', 0)
        return ms, stages

    for r in range(args.rounds):
        for rate in [1.0] + rates:
            ms, st = timed(rate)
            Tg = T if rate == 1.0 else eng.stretched_frames(T, rate)
            print('(b) rate {}, round {}: {} frames (T\' / T = {:.3f}), {:.3f} ms per batch; {}'.format(
                rate, r + 1, Tg, Tg / T, ms, ' '.join('{} {:.3f}'.format(k, v) for k, v in st.items())), flush=True)
eng.close()
