#!/usr/bin/env python3
"""The join (tts_join) on an MI355X at bench.py's shape: 64 rows of 275 000 samples joined into 8 texts of 8 pieces
each, with fades of 110 samples (5 ms at 22 050 Hz) and gaps of both signs -- a cross-fade of 110 samples and a pause of 7 717
(350 ms) in turn.  Every piece starts at an odd sample of its row, so no source is aligned with its place in the output.  Device
time per call from profile stage "join" over `--calls` calls enqueued back to back after three warm-up calls (5000 calls: a window of 0.15 s and more), twice -- on one set
of buffers (142 MB: it fits the 256 MiB last-level cache, so a call may find the previous call's lines there) and rotating over
`--sets` sets (three: 427 MB, every call's bytes come from HBM and go there).

    python tools/join_bench.py [--calls 5000] [--rows 64] [--samples 275000] [--texts 8] [--fade 110]

Beside the time: the bytes a call must move -- 4 read and 4 written per output sample, 8 B times G * N_out, the zeros of the pauses
and of the rows' ends counted as written and read -- per second and as a fraction of the HBM peak (8 TB/s).  The kernel computes
nothing but at the edges of the pieces, so that fraction is its figure of merit."""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=5000)
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
ap.add_argument('--texts', type=int, default=8)
ap.add_argument('--fade', type=int, default=110)
ap.add_argument('--sets', type=int, default=3)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
HBM_PEAK = 8.0e12

B, n, G, fade = args.rows, args.samples, args.texts, args.fade
eng = sstts.Engine()
rng = np.random.default_rng(0)
row = (0.1 * rng.standard_normal(n)).astype(np.float32)
xs = [eng.empty((B, n)) for _ in range(args.sets)]
for x in xs:
    for b in range(B):   # (filled row by row: one row of host random numbers)
        eng._check(eng.lib.tts_memcpy_h2d(eng.handle, x.ptr + b * row.nbytes, np.roll(row, 37 * b).ctypes.data, row.nbytes))
pieces = np.array([(b, 1 + 2 * (b % 5), n - 64 - b, -fade if b % 2 == 0 else 7717) for b in range(B)], dtype=np.int32)
groups = np.ascontiguousarray(np.arange(B) * G // B, dtype=np.int32)
n_out = eng.join_plan((B, n), pieces, groups, fade)
N_out = (int(n_out.max()) + 3) // 4 * 4
outs = [eng.empty((G, N_out)) for _ in range(args.sets)]
eng.set_option('profile', 1)
p_groups = groups.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
nbytes = 8.0 * G * N_out

print('{} rows of {} samples -> {} texts of up to {} samples (N_out {}), fade {}, {} launch(es) per call, {:.1f} MB per call'.format(
    B, n, G, int(n_out.max()), N_out, fade, -(-B // 128), nbytes / 1e6), flush=True)


def call(k):
    eng._check(eng.lib.tts_join(eng.handle, xs[k].ptr, B, n, pieces.ctypes.data, B, p_groups, G, fade, N_out, outs[k].ptr))


for name, sets in (('one set', 1), ('{} sets'.format(args.sets), args.sets)):
    for rep in range(2):
        for k in range(3):
            call(k % sets)
        eng.profile_reset()
        for k in range(args.calls):
            call(k % sets)
        ms, launches = eng.profile_get('join')
        per = ms / args.calls
        print('join {:8s} run {}: {:8.4f} ms per call, {:5.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            name, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)
