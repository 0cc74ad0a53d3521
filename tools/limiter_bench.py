#!/usr/bin/env python3
"""The limiter stage (tts_limit, tts_true_peak) on an MI355X at bench.py's shape: 64 utterances of 275 000 samples,
a look-ahead of 110 samples (5 ms at 22 050 Hz), in both modes (sample peaks and 4x interpolated peaks).  Device time per call from
profile stage "limiter" over `--calls` calls after three warm-up calls, twice each, on two inputs:

    skip   nothing over the ceiling: every tile computes its required gains, finds them all 1 and ends -- one read of the rows
    over   about 1 % of the samples over the ceiling (the ceiling is the 99th percentile of |x|), spread evenly: every tile runs
           the minimum, the mean and the copy.  The limiter works in place, so the rows are uploaded afresh in front of every call
           (outside the profiled span)

    python tools/limiter_bench.py [--calls 50] [--batch 64] [--samples 275000] [--lookahead 110]

Beside the time: the bytes a call must move -- the rows once on the skip path; read, written to the workspace copy, read back and
written in place on the other -- per second and as a fraction of the HBM peak (8 TB/s), and for the over path the LDS reads of
the mean (2 L + 1 doubles per sample) per second."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=50)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
ap.add_argument('--lookahead', type=int, default=110)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
HBM_PEAK = 8.0e12

B, n, L = args.batch, args.samples, args.lookahead
eng = sstts.Engine()
rng = np.random.default_rng(0)
row = (0.1 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(np.arange(n) * (2.0 * np.pi * 3.1 / 22050)))).astype(np.float32)
host = np.stack([np.roll(row, 37 * b) for b in range(B)])
ceiling_over = float(np.percentile(np.abs(host), 99.0))
ceiling_skip = 2.0 * float(np.abs(host).max())
x = eng.to_device(host)
stats = eng.empty((B, 2), np.float64)
tp = eng.empty((B,), np.float64)
eng.set_option('profile', 1)


def timed(name, call, nbytes, restore, lds_bytes=0.0):
    for rep in range(2):
        for _ in range(3):
            if restore:
                x.copy_from(host)
            eng._check(call())
        eng.profile_reset()
        for _ in range(args.calls):
            if restore:
                x.copy_from(host)
            eng._check(call())
        ms, launches = eng.profile_get('limiter')
        per = ms / args.calls
        line = '{:14s} run {}: {:8.4f} ms per call, {:4.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            name, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK)
        if lds_bytes:
            line += ', mean: {:6.2f} TB/s from LDS'.format(lds_bytes / (per * 1e-3) / 1e12)
        print(line, flush=True)


print('B = {}, n = {}, look-ahead {}: {} tiles per utterance, {} bytes of LDS per workgroup'.format(B, n, L, -(-n // 2048), 8 * (3 * 2048 + 10 * L + 11)))
rows = 4.0 * B * n
timed('true_peak', lambda: eng.lib.tts_true_peak(eng.handle, x.ptr, B, n, None, tp.ptr, None), rows, False)
for oversample in (1, 4):
    timed('skip, mode %d' % oversample, lambda: eng.lib.tts_limit(eng.handle, x.ptr, B, n, None, ceiling_skip, L, oversample, stats.ptr), rows, False)
    timed('over, mode %d' % oversample, lambda: eng.lib.tts_limit(eng.handle, x.ptr, B, n, None, ceiling_over, L, oversample, stats.ptr), 4.0 * rows, True,
          lds_bytes=8.0 * (2 * L + 1) * B * n)
    st = stats.to_host().view(sstts._hip.LIMIT_RECORD).reshape(B)
    print('    last call: {:.2f} % of the samples over, {:.2f} % limited, smallest gain {:.4f}; |x| <= {:.6f} = the ceiling {:.6f}'.format(
        100.0 * st['over'].sum() / (B * n), 100.0 * st['limited'].sum() / (B * n), st['min_gain'].min(), float(np.abs(x.to_host()).max()), ceiling_over))
