#!/usr/bin/env python3
"""The loudness stage (tts_loudness, tts_loudness_normalize) on an MI355X at bench.py's shape: 64 utterances of
275 000 samples at 22 050 Hz.  Device time per call from profile stage "loudness" over `--calls` calls enqueued back to back after
three warm-up calls, twice each: the measurement alone, and the normaliser (the measurement, the peak, the gain and the scaling
pass, in place -- the waveforms are at the target from the first call on, so every timed call does the same work).

    python tools/loudness_bench.py [--calls 200] [--batch 64] [--samples 275000] [--sampling-rate 22050]

Beside the time: the bytes a call must move -- the samples read twice by the measurement (passes 1 and 3), and by the normaliser
once more for the peak and read and written by the scaling -- per second and as a fraction of the HBM peak (8 TB/s).  The passes
are bound by the latency of the recurrence, not by memory: the fraction says how far from a memory-bound pass they are."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
ap.add_argument('--sampling-rate', type=int, default=22050)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
HBM_PEAK = 8.0e12

B, n, sr = args.batch, args.samples, args.sampling_rate
eng = sstts.Engine()
rng = np.random.default_rng(0)
row = (0.1 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(np.arange(n) * (2.0 * np.pi * 3.1 / sr)))).astype(np.float32)
x = eng.empty((B, n))
for b in range(B):   # (filled utterance by utterance: one row of host random numbers)
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, x.ptr + b * row.nbytes, (np.roll(row, 37 * b) * np.float32(1.0 + 0.05 * b)).ctypes.data,
                                      row.nbytes))
z = eng.empty((B,), np.float64)
g = eng.empty((B,), np.float64)
eng.set_option('profile', 1)


def timed(name, call, nbytes):
    for rep in range(2):
        for _ in range(3):
            eng._check(call())
        eng.profile_reset()
        for _ in range(args.calls):
            eng._check(call())
        ms, launches = eng.profile_get('loudness')
        per = ms / args.calls
        print('{:10s} run {}: {:8.4f} ms per call, {:5.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            name, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)


print('B = {}, n = {}, sampling rate {}: {} steps, {} blocks, {} segments per utterance'.format(B, n, sr, n // (sr // 10), max(0, n // (sr // 10) - 3),
                                                                                                8 * (n // (sr // 10))))
timed('measure', lambda: eng.lib.tts_loudness(eng.handle, x.ptr, B, n, None, sr, z.ptr, None), 2.0 * 4 * B * n)
timed('normalize', lambda: eng.lib.tts_loudness_normalize(eng.handle, x.ptr, B, n, None, sr, -23.0, 1.0, z.ptr, g.ptr), 5.0 * 4 * B * n)
lufs = -0.691 + 10.0 * np.log10(z.to_host())
print('loudness after the last call: {:.4f} .. {:.4f} LUFS, gains {:.6f} .. {:.6f}'.format(lufs.min(), lufs.max(), g.to_host().min(), g.to_host().max()))
