#!/usr/bin/env python3
"""End-of-speech stopping (tts_set_end_of_speech) at bench.py's shape: 64 utterances x 150 ids, 200 decoder
steps (1000 frames), 60 Griffin-Lim iterations, seeded phases, peak normalisation, calls back to back on device-resident ids;
ms per batch from a host clock around `--steps` calls that end in one synchronise, after `--warmup` calls.

    python tools/eos_bench.py [--steps 20] [--warmup 3] [--rounds 2] [--shares 0.45,0.65,0.85] [--embedding-scale 64]
                              [--id-sets 24]

Every call synthesises ANOTHER batch of sentences: `--id-sets` device-resident id arrays (more than steps + warm-up, and more
than the 16 entries of the handle's plan store) are taken in turn, so that with the setting on every call finds lengths it has
not seen -- it plans both cuts and builds its window tables in the call, as a server's calls do.  The "same sentences" lines
of (c) repeat one batch instead: every call then finds the previous call's plans and tables, which flatters the feature.

Lines, the runs of one section alternating within a round:
  (a) the setting off;  (b) on with a threshold below every value -- nothing is trimmed, the call is the uniform call plus the
      detection launches, the read-back of the lengths (the host waits for the post-net) and the plan lookup;
  (c) on with thresholds that trim: candidate thresholds are tried with tts_speech_frames on the first batch's `linear` (a
      grid of the normalised scale), and the ones whose frames' share of the padded batch comes nearest to `--shares` are run
      -- ms per batch beside the mean share of the timed calls, the Griffin-Lim stage times beside (a)'s;
  (d) tts_speech_frames alone on the (64, 1000, 1025) `linear`: device time per call against its bytes over the HBM peak.
The seeded synthetic weights make 64 nearly identical utterances; `--embedding-scale` (the tests' device) spreads them so that
one threshold gives a spread of lengths.  It applies to every line alike."""
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
ap.add_argument('--shares', default='0.45,0.65,0.85')
ap.add_argument('--embedding-scale', type=float, default=64.0)
ap.add_argument('--keep-ms', type=float, default=100.0)
ap.add_argument('--id-sets', type=int, default=24)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
P = importlib.import_module('single-speaker-tts_amd.tacotron.params')
W = importlib.import_module('single-speaker-tts_amd.tacotron.weights')
B, TS, N_STEPS, N_ITER = 64, 150, 200, 60
WIN, HOP, N_FFT = 1102, 275, 2048
REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3
HBM_PEAK = 8.0e12   # bytes per second, MI355X

hp = P.ModelParams()
weights = W.synthetic_weights(0, hp)
weights['encoder/embedding'] = np.ascontiguousarray(weights['encoder/embedding'] * np.float32(args.embedding_scale))
eng = sstts.Engine(hp)
eng.load_weights(weights)
rng = np.random.default_rng(1234)
id_sets = []
for k in range(max(1, args.id_sets)):
    ids_h = rng.integers(2, hp.vocabulary_size, (B, TS)).astype(np.int32)
    for b in range(B):   # sentences of different lengths, padded; another spread in every set
        ids_h[b, TS - 1 - (b * 2 + 7 * k) % 100:] = 0
    id_sets.append(eng.to_device(ids_h))
T, F = N_STEPS * hp.reduction, 1 + N_FFT // 2
wav = eng.empty((B, HOP * (T - 1)))
lin = eng.empty((B, T, F))
keep = sstts._hip.silence_keep_frames(int(args.keep_ms / 1000 * hp.sampling_rate), HOP)
calls = [0]


def step(stop, want_linear=False, fresh=True):
    calls[0] += 1
    ids = id_sets[calls[0] % len(id_sets)] if fresh else id_sets[0]
    return eng.synthesize(ids, N_STEPS, REF_DB, MAX_DB, POWER, N_ITER, WIN, HOP, seed=calls[0], peak_normalize=True, wav=wav,
                          want_linear=lin if want_linear else False, stop_at_silence=stop)


def timed(stop, fresh=True):
    """(ms per batch, the lengths of the timed calls, stage ms per batch)"""
    lengths = []
    for _ in range(args.warmup):
        step(stop, fresh=fresh)
    eng.set_option('profile', 1)
    eng.profile_reset()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step(stop, fresh=fresh)
        lengths.append(out['n_frames'] if stop is not None else None)
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    stages = {s: eng.profile_get(s)[0] / args.steps for s in ('postnet', 'speech_end', 'gl_iter', 'gl_final')}
    eng.set_option('profile', 0)
    return ms, np.stack(lengths) if stop is not None else eng.synth_frames(B)[None], stages


def fmt(stages):
    return ' '.join('{} {:.3f}'.format(k, v) for k, v in stages.items())


# ---- (a) / (b)
BELOW = (-101.0, 0)   # the clip of the de-normalisation keeps every value at or above ref_db - |ref_db| - |max_db| = -99.89 dB
base = []
for r in range(args.rounds):
    ms, n, st = timed(None)
    base.append(ms)
    print('(a) off, round {}: {:.3f} ms per batch; {}'.format(r + 1, ms, fmt(st)), flush=True)
    ms, n, st = timed(BELOW)
    assert (n == T).all()
    print('(b) on, threshold below every value, round {}: {:.3f} ms per batch; {}'.format(r + 1, ms, fmt(st)), flush=True)
a_ms = min(base)

# ---- (c): thresholds from the batch's own linear spectrograms
step(None, want_linear=True, fresh=False)
eng.synchronize()
min_frames = (N_FFT // 2) // HOP + 2
n_dev, last_dev = eng.empty((B,), np.int32), eng.empty((B,), np.int32)


def lengths_at(x_norm, keep_frames):
    eng._check(eng.lib.tts_speech_frames(eng.handle, lin.data_ptr(), B, T, F, F, float(x_norm), keep_frames, min_frames, n_dev.data_ptr(),
                                         last_dev.data_ptr()))
    return n_dev.to_host()


# candidate thresholds on a grid of the normalised scale; the frames' share of the padded batch at each
cands = []
for x in np.linspace(0.0, 1.0, 201):
    n = lengths_at(x, keep)
    cands.append((float(n.sum()) / (B * T), float(x), n))
for want in [float(s) for s in args.shares.split(',')]:
    share, x, n = min(cands, key=lambda c: abs(c[0] - want))
    thr_db = (x - 1.0) * (abs(REF_DB) + abs(MAX_DB)) + REF_DB
    for r in range(args.rounds):
        for fresh in (True, False):
            ms, got, st = timed((thr_db, keep), fresh=fresh)
            distinct = len({tuple(v) for v in got.tolist()})
            print('(c) on, threshold {:.2f} dB (+{} frames kept), {}, round {}: {} length vectors in {} calls, lengths {} .. {} (mean {:.0f}), '
                  'frames\' share {:.3f}: {:.3f} ms per batch ((a) {:.3f}); {}'.format(
                      thr_db, keep, 'other sentences every call' if fresh else 'same sentences', r + 1, distinct, len(got), got.min(),
                      got.max(), got.mean(), float(got.mean()) / T, ms, a_ms, fmt(st)), flush=True)

# ---- (d): the stage alone
eng.set_option('profile', 1)
for rep in range(2):
    eng.profile_reset()
    for _ in range(20):
        lengths_at(0.5, 0)
    ms, launches = eng.profile_get('speech_end')
    ms /= 20
    nbytes = 4.0 * B * T * F
    print('(d) tts_speech_frames on ({}, {}, {}): {:.1f} us per call ({} launches), {:.0f} MB -> {:.0f} GB/s, {:.0f} % of the {:.0f} TB/s HBM peak '
          '({:.1f} us at the peak)'.format(B, T, F, ms * 1e3, launches // 20, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e9,
                                           100.0 * nbytes / (ms * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12, nbytes / HBM_PEAK * 1e6))
eng.set_option('profile', 0)
eng.close()
