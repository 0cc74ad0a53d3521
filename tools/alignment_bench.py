#!/usr/bin/env python3
"""The attention diagnostics (tts_alignment_stats) on an MI355X at bench.py's shape and two beside it: 200 decoder
steps x 64 utterances x 100 positions, 200 x 64 x 256 and 200 x 1 x 100.  Device time per call from profile stage "alignment" over
`--calls` calls enqueued back to back after three warm-up calls, twice each, and the wall time per call of the same loop (what a
caller that enqueues nothing else pays: the launches).

    python tools/alignment_bench.py [--calls 200] [--shapes 200x64x100,200x64x256,200x1x100]

Beside the time: the bytes a call must move -- the alignments, read once -- per second and as a fraction of the HBM peak (8 TB/s).
The stage is two launches per 64 utterances and is bound by launch latency and the sequential focus walk, not by memory: the
fraction says how far from a memory-bound pass it is."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--shapes', default='200x64x100,200x64x256,200x1x100')
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')
HBM_PEAK = 8.0e12

eng = sstts.Engine()
eng.set_option('profile', 1)
for shape in args.shapes.split(','):
    S, B, Ts = (int(v) for v in shape.split('x'))
    rng = np.random.default_rng([S, B, Ts])
    x = rng.standard_normal((S, B, Ts)).astype(np.float32)
    x[np.arange(S)[:, None], np.arange(B)[None, :], (np.arange(S)[:, None] * Ts // (2 * S) + np.arange(B)[None, :]) % Ts] += 4.0
    w = np.exp(x - x.max(axis=2, keepdims=True))
    ali = eng.to_device((w / w.sum(axis=2, keepdims=True)).astype(np.float32))
    stats = eng.empty((B,), H.ALIGNMENT_RECORD)
    n_sent = np.full(B, max(1, (3 * Ts) // 4), np.int32)
    p_sent = n_sent.ctypes.data_as(H.POINTER(H.c_int32))

    def call():
        return eng.lib.tts_alignment_stats(eng.handle, ali.ptr, S, B, Ts, p_sent, None, stats.ptr, None, None, None)

    nbytes = 4.0 * S * B * Ts
    for rep in range(2):
        for _ in range(3):
            eng._check(call())
        eng.synchronize()
        eng.profile_reset()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            eng._check(call())
        eng.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.calls
        ms, launches = eng.profile_get('alignment')
        per = ms / args.calls
        print('{:>12s} run {}: {:8.4f} ms per call on the device, {:8.4f} ms wall, {:4.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            shape, rep, per, wall, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)
    rec = stats.to_host()
    print('{:>12s} records: end_step {} .. {}, mean focus {:.4f}, off_text {}'.format(
        shape, rec['end_step'].min(), rec['end_step'].max(), float(np.mean(rec['focus_sum'] / rec['n_steps'])), int(rec['off_text'].sum())), flush=True)
    ali.free()
    stats.free()
