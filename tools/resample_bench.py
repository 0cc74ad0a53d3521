#!/usr/bin/env python3
"""The resampler (tts_resample) on an MI355X at bench.py's shape: 64 utterances of 275 000 samples, at the ratios
of a pitch of four semitones down and up (2 ** (4 / 12), 2 ** (-4 / 12)), 0.5 and 2.  Device time per call from profile stage
"resample" over `--calls` calls enqueued back to back after three warm-up calls (1000 calls of about half a millisecond: a
timed window of about half a second), twice per ratio.

    python tools/resample_bench.py [--calls 1000] [--ratios up4,down4,0.5,2] [--batch 64] [--samples 275000]

Beside the time, per ratio:
  - the input read once plus the output written, as bytes per second and as a fraction of the HBM peak (8 TB/s): what a
    memory-bound pass would be held to;
  - the double FMAs the arithmetic asks for -- per output and utterance one per tap, (32769 - off) / step on each wing, plus the
    weight's own FMA per tap shared by the eight utterances of a group -- per second, and as a fraction of the vector FP64 peak
    (78.6 TFLOP/s = 39.3 T FMA/s);
  - the table bytes the taps ask for (16 per tap and group of eight utterances) per second.  A DERIVED figure, from the tap
    counts: no counter is read, and it says nothing about which cache answered.
The table of a ratio is built and uploaded by the first call at that ratio; that call is among the warm-up calls."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=1000)
ap.add_argument('--ratios', default='up4,down4,0.5,2')
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')
NAMED = {'up4': 2.0 ** (-4.0 / 12.0), 'down4': 2.0 ** (4.0 / 12.0)}   # the ratio the resampler runs at for that pitch
HBM_PEAK, FMA_PEAK = 8.0e12, 39.3e12
NWIN = 32769

B, n = args.batch, args.samples
eng = sstts.Engine()
row = np.random.default_rng(0).standard_normal(n).astype(np.float32)
x = eng.empty((B, n))
for b in range(B):   # (filled utterance by utterance: one row of host random numbers)
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, x.ptr + b * row.nbytes, np.roll(row, 37 * b).ctypes.data, row.nbytes))
eng.set_option('profile', 1)
for name in args.ratios.split(','):
    rho = NAMED[name] if name in NAMED else float(name)
    N_out = H.resampled_length(n, rho)
    out = eng.empty((B, N_out))
    scale = min(1.0, rho)
    step = int(scale * 512)
    taps = 2.0 * (NWIN / step)                      # per output, both wings (off is spread evenly: the mean of (32769 - off) / step)
    fmas = N_out * taps * (B + -(-B // 8))          # one per utterance, and the weight's once per group of eight
    table_bytes = 16.0 * N_out * taps * -(-B // 8)
    io_bytes = 4.0 * B * (n + N_out)
    for rep in range(2):
        for _ in range(3):
            eng._check(eng.lib.tts_resample(eng.handle, x.ptr, B, n, None, rho, N_out, out.ptr))
        eng.profile_reset()
        for _ in range(args.calls):
            eng._check(eng.lib.tts_resample(eng.handle, x.ptr, B, n, None, rho, N_out, out.ptr))
        ms, launches = eng.profile_get('resample')
        s = ms * 1e-3 / args.calls
        print('tts_resample {} x {} -> {} (ratio {} = {:.6f}, step {}, {:.0f} taps): {:.3f} ms per call ({} launch); in + out {:.0f} MB '
              '-> {:.2f} TB/s = {:.3f} of the HBM peak; {:.2f} G double FMA -> {:.2f} T FMA/s = {:.3f} of the FP64 vector peak; '
              'table bytes asked for {:.1f} GB -> {:.2f} TB/s (derived)'.format(B, n, N_out, name, rho, step, taps, s * 1e3, launches // args.calls,
                                                            io_bytes / 1e6, io_bytes / s / 1e12, io_bytes / s / HBM_PEAK, fmas / 1e9,
                                                            fmas / s / 1e12, fmas / s / FMA_PEAK, table_bytes / 1e9, table_bytes / s / 1e12),
              flush=True)
    out.free()
eng.set_option('profile', 0)
x.free()
eng.close()
