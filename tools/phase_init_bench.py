#!/usr/bin/env python3
"""Estimated initial phases for Griffin-Lim (option "gl_init") on an MI355X: the pass alone, the iteration
count it buys, and whole calls with and without it.

    python tools/phase_init_bench.py [--steps 20] [--warmup 3] [--rounds 2] [--n-star N] [--skip-kernels] [--skip-quality] [--skip-calls]

Lines:
  (a) tts_phase_estimate_rows (time-major rows of 1056 floats, the call pipeline's buffer) and tts_phase_estimate ((F, T), the
      public layout) at 64 x 1000 x 1025 and at B = 1: device time per call (profile stage "phase_init"), the launches, and
      the bytes the pass moves -- the magnitudes read twice (compose, apply), the phases written time-major, read and written
      again by the transpose, the chunk maps and starts (10 bytes per bin and chunk, written and read once); the public layout
      adds a transpose of the magnitudes -- against the 8 TB/s HBM peak of the data sheet;
  (b) N*: the smallest iteration count at which the mse (tts_griffin_lim's, reference audio/synthesis.py:112) from the estimated
      start is at or below the mse after 60 iterations from default_rng(0) phases, on frames 0:400 of the shipped spectrogram
      (tests/golden/reference_linear_spec_post_215k.npz); 12 by the float64 oracle on the CPU;
  (c) whole calls at bench.py's shape -- 64 utterances x 150 ids, 200 decoder steps (1000 frames), seeded phases, peak
      normalisation, calls back to back on device-resident ids (the pipelined stream) -- and one utterance at a time with the
      pipeline off: 60 iterations with the option off (the parent's path), N* iterations with the option on, alternating within
      a round; ms per batch from a host clock around `--steps` calls that end in one synchronise, and the stage times."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--rounds', type=int, default=2)
ap.add_argument('--n-star', type=int, default=None, help='iterations of the calls with the option on (default: what (b) finds, else 12)')
ap.add_argument('--skip-kernels', action='store_true')
ap.add_argument('--skip-quality', action='store_true')
ap.add_argument('--skip-calls', action='store_true')
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
P = importlib.import_module('single-speaker-tts_amd.tacotron.params')
W = importlib.import_module('single-speaker-tts_amd.tacotron.weights')
B, TS, N_STEPS, N_ITER = 64, 150, 200, 60
WIN, HOP, N_FFT = 1102, 275, 2048
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3
HBM_PEAK = 8.0e12   # bytes per second, the data sheet's

hp = P.ModelParams()
eng = sstts.Engine(hp)
T, F, FP = N_STEPS * hp.reduction, 1 + N_FFT // 2, 1056
CHUNK = eng.phase_chunk_frames()


def shipped(t0, t1):
    """frames t0:t1 of the shipped spectrogram, de-normalised as inference does it (tests/momentum_oracle.py): (1025, n) float32"""
    from oracle import audio_oracle as A
    spec = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_linear_spec_post_215k.npz'))['linear_spec']
    lin = np.ascontiguousarray(spec[0, :, t0:t1, 0].T)
    return A.linear_to_magnitude(lin, REF_DB, MAX_DB, POWER).astype(np.float32)


# ---- (a) the pass alone
if not args.skip_kernels:
    speech = shipped(0, 400)
    frame = np.zeros((T, FP), np.float32)
    frame[:, :F] = np.tile(speech, (1, 3))[:, :T].T      # speech-like peaks (a pass over noise finds a peak every third bin)
    for nb in (B, 1):
        rows_in = eng.empty((nb, T, FP))
        cols_in = eng.empty((nb, F, T))
        out = eng.empty((nb, F, T))
        part = frame[:, :F].T.copy()
        for b in range(nb):
            eng._check(eng.lib.tts_memcpy_h2d(eng.handle, rows_in.ptr + b * frame.nbytes, frame.ctypes.data, frame.nbytes))
            eng._check(eng.lib.tts_memcpy_h2d(eng.handle, cols_in.ptr + b * part.nbytes, part.ctypes.data, part.nbytes))
        n_chunks = -(-T // CHUNK)
        bins = float(nb) * F * T
        moved_rows = 4.0 * bins * (2 + 3) + 2 * 10.0 * nb * F * (n_chunks - 1)
        calls = {
            'tts_phase_estimate_rows [B][T][1056]': (lambda: eng.lib.tts_phase_estimate_rows(eng.handle, rows_in.ptr, nb, T, FP, None, N_FFT, HOP, out.ptr), moved_rows),
            'tts_phase_estimate      [B][F][T]   ': (lambda: eng.lib.tts_phase_estimate(eng.handle, cols_in.ptr, nb, T, None, N_FFT, HOP, out.ptr), moved_rows + 8.0 * bins),
        }
        eng.set_option('profile', 1)
        for name, (call, nbytes) in calls.items():
            for rep in range(2):
                for _ in range(3):
                    eng._check(call())
                eng.profile_reset()
                for _ in range(20):
                    eng._check(call())
                ms, launches = eng.profile_get('phase_init')
                ms /= 20
                bps = nbytes / (ms * 1e-3)
                print('(a) {} B = {}: {} frames in chunks of {}, {:.1f} us per call ({} launches), {:.0f} MB moved -> {:.2f} TB/s, {:.2f} of the '
                      '{:.0f} TB/s HBM peak'.format(name, nb, T, CHUNK, ms * 1e3, launches // 20, nbytes / 1e6, bps / 1e12, bps / HBM_PEAK,
                                                    HBM_PEAK / 1e12), flush=True)
        eng.set_option('profile', 0)
        for a in (rows_in, cols_in, out):
            a.free()

# ---- (b) the iteration count the estimate buys
n_star = args.n_star
if not args.skip_quality:
    mag = shipped(0, 400)[None]
    init = np.random.default_rng(0).random(mag.shape).astype(np.float32)
    mse = lambda n_iter, **kw: float(eng.griffin_lim(mag, n_iter, WIN, HOP, N_FFT, **kw)[1].to_host()[0])
    rand = {n: mse(n, init_phase=init) for n in (1, 5, 10, 20, 30, 60)}
    print('(b) random start    : ' + ' '.join('{}: {:.3e}'.format(n, v) for n, v in rand.items()), flush=True)
    est = {n: mse(n, phase_init='estimate') for n in range(1, 31)}
    print('(b) estimated start : ' + ' '.join('{}: {:.3e}'.format(n, est[n]) for n in (1, 5, 10, 20, 30)) +
          ' 60: {:.3e}'.format(mse(60, phase_init='estimate')), flush=True)
    found = [n for n in sorted(est) if est[n] <= rand[60]]
    print('(b) N* = {} (the first iteration at or below the random start\'s {:.3e} at 60; 12 by the CPU oracle)'.format(
        found[0] if found else 'beyond 30', rand[60]), flush=True)
    if n_star is None and found:
        n_star = found[0]
n_star = 12 if n_star is None else n_star

# ---- (c) whole calls
if not args.skip_calls:
    eng.load_weights(W.synthetic_weights(0, hp))
    rng = np.random.default_rng(1234)
    for nb, pipeline in ((B, 1), (1, 0)):
        ids_h = rng.integers(2, hp.vocabulary_size, (nb, TS)).astype(np.int32)
        ids_h[:, -1] = 1
        ids = eng.to_device(ids_h)
        wav = eng.empty((nb, HOP * (T - 1)))
        eng.set_option('pipeline', pipeline)
        calls = [0]

        def timed(phase_init, n_iter):
            def step():
                calls[0] += 1
                eng.synthesize(ids, N_STEPS, REF_DB, MAX_DB, POWER, n_iter, WIN, HOP, seed=calls[0], peak_normalize=True, wav=wav,
                               phase_init=phase_init)
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
            stages = {s: eng.profile_get(s)[0] / args.steps for s in ('postnet', 'phase_init', 'gl_iter', 'gl_final')}
            eng.set_option('profile', 0)
            return ms, stages

        for r in range(args.rounds):
            for phase_init, n_iter in (('random', N_ITER), ('estimate', n_star), ('estimate', N_ITER)):
                ms, st = timed(phase_init, n_iter)
                print('(c) B = {} pipeline {} round {}: {:8s} start, {:2d} iterations: {:.3f} ms per batch; {}'.format(
                    nb, pipeline, r + 1, phase_init, n_iter, ms, ' '.join('{} {:.3f}'.format(k, v) for k, v in st.items())), flush=True)
        eng.set_option('pipeline', 1)
        ids.free()
        wav.free()
eng.close()
