#!/usr/bin/env python3
"""The timing marks' search (tts_token_times) on an MI355X at bench.py's shape and three beside it: 200 decoder
steps x 64 utterances x 100 positions, 200 x 64 x 256, 200 x 1 x 100 and 200 x 64 x 300 (whose directions do not fit LDS), each
beside tts_alignment_stats at the same shape.  Device time per call from profile stage "alignment" over `--calls` calls enqueued
back to back after three warm-up calls, twice each, and the wall time per call of the same loop.

    python tools/marks_bench.py [--calls 200] [--shapes 200x64x100,200x64x256,200x1x100,200x64x300] [--max-jump 4]

The search is a chain: S rows, each a barrier and an LDS round trip behind the one before, then S dependent reads of the walk back.
Beside the time: the time per step of the chain, which is what bounds it -- not the bytes (the alignments, read once) and not the
arithmetic."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--shapes', default='200x64x100,200x64x256,200x1x100,200x64x300')
ap.add_argument('--max-jump', type=int, default=4)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')

eng = sstts.Engine()
eng.set_option('profile', 1)
for shape in args.shapes.split(','):
    S, B, Ts = (int(v) for v in shape.split('x'))
    rng = np.random.default_rng([S, B, Ts])
    x = rng.standard_normal((S, B, Ts)).astype(np.float32)
    x[np.arange(S)[:, None], np.arange(B)[None, :], (np.arange(S)[:, None] * Ts // (2 * S) + np.arange(B)[None, :]) % Ts] += 4.0
    w = np.exp(x - x.max(axis=2, keepdims=True))
    ali = eng.to_device((w / w.sum(axis=2, keepdims=True)).astype(np.float32))
    records = eng.empty((B,), H.ALIGNMENT_RECORD)
    start = eng.empty((B, Ts + 1), np.int32)
    stats = eng.empty((B,), H.TOKEN_TIMES_RECORD)
    n_sent = np.full(B, max(1, (3 * Ts) // 4), np.int32)
    p_sent = n_sent.ctypes.data_as(H.POINTER(H.c_int32))

    def search():
        return eng.lib.tts_token_times(eng.handle, ali.ptr, S, B, Ts, p_sent, None, args.max_jump, start.ptr, None, stats.ptr)

    def diagnostics():
        return eng.lib.tts_alignment_stats(eng.handle, ali.ptr, S, B, Ts, p_sent, None, records.ptr, None, None, None)

    for name, call in (('token_times', search), ('alignment_stats', diagnostics)):
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
            print('{:>12s} {:>15s} run {}: {:8.4f} ms per call on the device, {:8.4f} ms wall, {:4.1f} launches, {:6.3f} us per decoder step'.format(
                shape, name, rep, per, wall, launches / args.calls, 1e3 * per / S), flush=True)
    rec = stats.to_host()
    print('{:>12s} records: last {} .. {}, jumps {}, skipped {}, agree {:.3f} of the steps'.format(
        shape, rec['last'].min(), rec['last'].max(), int(rec['jumps'].sum()), int(rec['skipped'].sum()),
        float(np.mean(rec['agree'] / rec['n_steps']))), flush=True)
    for a in (ali, records, start, stats):
        a.free()
