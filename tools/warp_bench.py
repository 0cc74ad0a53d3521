#!/usr/bin/env python3
"""The prosody warp (tts_warp_magnitudes) on an MI355X beside the uniform stretch it contains: 64 x 1025 x 1000
magnitudes at one rate (default 0.8: step 52429), the rows cut into one, four and sixteen segments of equal length that all carry
that step and gain 1 -- so every variant reads the same source frames and writes (up to a frame per segment) the same output as
tts_stretch_magnitudes at that rate, which is the yardstick: it moves the same bytes.  Device time per call from the profile
stages "warp" and "stretch" over `--calls` calls enqueued back to back after three warm-up calls, twice.

    python tools/warp_bench.py [--calls 200] [--rows 64] [--bins 1025] [--frames 1000] [--step 52429]

Beside the time: the bytes a call must move -- 4 per source element read once and 4 per output element written, the zeros of
the rows' ends included -- per second and as a fraction of the HBM peak (8 TB/s).  The 262 MB of the source and the 328 MB of
the output together do not fit the 256 MiB last-level cache: one set of buffers."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--bins', type=int, default=1025)
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--step', type=int, default=52429)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')
HBM_PEAK = 8.0e12

B, F, T, q = args.rows, args.bins, args.frames, args.step
rate = q / 65536.0
eng = sstts.Engine()
rng = np.random.default_rng(0)
plane = rng.random((F, T)).astype(np.float32)
mag = eng.empty((B, F, T))
for b in range(B):   # (filled row by row: one plane of host random numbers)
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, mag.ptr + b * plane.nbytes, np.roll(plane, 37 * b, axis=1).copy().ctypes.data, plane.nbytes))
T_st = eng.stretched_frames(T, rate)
eng.set_option('profile', 1)
print('{} x {} x {} at rate {:.4f} (step {}): the stretch writes {} frames per row'.format(B, F, T, rate, q, T_st), flush=True)


def timed(stage, call, nbytes, what):
    for rep in range(2):
        for _ in range(3):
            call()
        eng.profile_reset()
        for _ in range(args.calls):
            call()
        ms, launches = eng.profile_get(stage)
        per = ms / args.calls
        print('{:28s} run {}: {:8.4f} ms per call, {:5.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            what, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)


out = eng.empty((B, F, T_st))
timed('stretch', lambda: eng._check(eng.lib.tts_stretch_magnitudes(eng.handle, mag.ptr, B, F, T, None, rate, T_st, out.ptr)),
      4.0 * B * F * (T + T_st), 'stretch_magnitudes')
out.free()
for k in (1, 4, 16):
    cuts = [T * i // k for i in range(k + 1)]
    seg = H.warp_segments([(b, cuts[i], cuts[i + 1] - cuts[i], 0, q, 1.0) for b in range(B) for i in range(k)])
    n_out = eng.warp_plan((B, F, T), seg)
    T_out = int(n_out.max())
    out = eng.empty((B, F, T_out))
    timed('warp', lambda: eng._check(eng.lib.tts_warp_magnitudes(eng.handle, mag.ptr, B, F, T, None, seg.ctypes.data, len(seg), T_out, out.ptr)),
          4.0 * B * F * (T + T_out), 'warp, {:2d} segments per row'.format(k))
    out.free()
