#!/usr/bin/env python3
"""The formant-preserving pitch stage (tts_shift_magnitudes) on an MI355X: 64 x 1025 x 1000 magnitudes at order 33 in
three forms -- all-copy (one segment per row at 65536 / 65536), one segment per row at +4 semitones, and sixteen segments per row
at mixed steps (a quarter of them copies) -- beside tts_stretch_magnitudes at rate 1, which moves the same bytes, and
tts_resample_segments at +4 semitones on the matching samples (64 x 275 000), the pass the stage replaces.  Device time per call
from the profile stages "shift", "stretch" and "resample" over `--calls` calls enqueued back to back after three warm-up calls,
twice.

    python tools/shift_bench.py [--calls 100] [--rows 64] [--bins 1025] [--frames 1000] [--order 33]

Beside the time: the bytes a call must move -- 4 per element read once and 4 per element written -- per second and as a fraction
of the HBM peak (8 TB/s), and for the computed forms the double-precision FMAs of the two cosine sums, 2 Q F per frame, per second
and as a fraction of the vector FP64 peak (78.6 TFLOP/s = 39.3 T FMA/s); the logarithm and the three exponentials of every element
are not counted.  The 262 MB of the source and of the output do not fit the 256 MiB last-level cache together: one set of buffers."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=100)
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--bins', type=int, default=1025)
ap.add_argument('--frames', type=int, default=1000)
ap.add_argument('--order', type=int, default=33)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')
HBM_PEAK = 8.0e12
FMA_PEAK = 39.3e12
HOP = 275

B, F, T, Q = args.rows, args.bins, args.frames, args.order
eng = sstts.Engine()
rng = np.random.default_rng(0)
plane = (rng.random((F, T)) + 1e-3).astype(np.float32)
mag = eng.empty((B, F, T))
for b in range(B):   # (filled row by row: one plane of host random numbers)
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, mag.ptr + b * plane.nbytes, np.roll(plane, 37 * b, axis=1).copy().ctypes.data, plane.nbytes))
eng.set_option('profile', 1)
print('{} x {} x {} at order {}'.format(B, F, T, Q), flush=True)


def timed(stage, call, nbytes, fmas, what):
    for rep in range(2):
        for _ in range(3):
            call()
        eng.profile_reset()
        for _ in range(args.calls):
            call()
        ms, launches = eng.profile_get(stage)
        per = ms / args.calls
        print('{:30s} run {}: {:8.4f} ms per call, {:5.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak, {:6.2f} T FMA/s = {:5.2f} % of the FP64 peak'.format(
            what, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK, fmas / (per * 1e-3) / 1e12,
            100.0 * fmas / (per * 1e-3) / FMA_PEAK), flush=True)


out = eng.empty((B, F, T))
moved = 8.0 * B * F * T
timed('stretch', lambda: eng._check(eng.lib.tts_stretch_magnitudes(eng.handle, mag.ptr, B, F, T, None, 1.0, T, out.ptr)), moved, 0.0, 'stretch_magnitudes, rate 1')
up = H.shift_step(4.0)
mixed = (up, H.shift_step(-3.0), H.SHIFT_UNITY, H.shift_step(7.0))
cuts = [T * i // 16 for i in range(17)]
forms = [('shift, all copies', [(b, 0, T, H.SHIFT_UNITY, H.SHIFT_UNITY) for b in range(B)]),
         ('shift, 1 segment per row, +4 st', [(b, 0, T, up, H.SHIFT_UNITY) for b in range(B)]),
         ('shift, 16 per row, mixed steps', [(b, cuts[i], cuts[i + 1] - cuts[i], mixed[i % 4], H.SHIFT_UNITY) for b in range(B) for i in range(16)])]
for what, rows in forms:
    seg = H.shift_segments(rows)
    eng.shift_plan((B, F, T), seg, None, Q)
    computed = sum(int(q['frames']) for q in seg if (int(q['pitch_step']), int(q['formant_step'])) != (H.SHIFT_UNITY, H.SHIFT_UNITY))
    timed('shift', lambda: eng._check(eng.lib.tts_shift_magnitudes(eng.handle, mag.ptr, B, F, T, None, seg.ctypes.data, len(seg), Q, out.ptr)),
          moved, 2.0 * Q * F * computed, what)
out.free()
mag.free()

n = HOP * T
wav = eng.empty((B, n))
row = (rng.random(n) - 0.5).astype(np.float32)
for b in range(B):
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, wav.ptr + b * row.nbytes, np.roll(row, 37 * b).copy().ctypes.data, row.nbytes))
ratio = 2.0 ** (-4.0 / 12.0)
rseg = H.resample_segment_list([(b, 0, n, ratio) for b in range(B)], B, n)[0]
N_out = int(eng.resample_segments_plan((B, n), rseg).max())
res = eng.empty((B, N_out))
timed('resample', lambda: eng._check(eng.lib.tts_resample_segments(eng.handle, wav.ptr, B, n, None, rseg.ctypes.data, len(rseg), N_out, res.ptr, None)),
      4.0 * B * (n + N_out), 0.0, 'resample_segments, +4 st')
