#!/usr/bin/env python3
"""The segment-wise resampler (tts_resample_segments) on an MI355X at bench.py's shape: 64 rows of 275 000
samples.  Device time per call from profile stage "resample" over `--calls` calls enqueued back to back after three warm-up
calls, twice per case:

  - all-copy: one segment per row at ratio 1.0 (what a row without a pitch costs inside a call with one);
  - one segment per row at 2 ** (-4 / 12), beside tts_resample on the same rows: its batched form (B = 64, a weight applied to
    eight rows) and the single-utterance form it runs at B = 1, times 64 -- the yardstick, since every row of a segment list
    carries its own ratios and a weight serves one sample;
  - four and sixteen segments per row with mixed ratios (copies, 2 ** (-4 / 12), 2 ** (3 / 12), 0.5).

    python tools/resample_segments_bench.py [--calls 100] [--batch 64] [--samples 275000] [--out profiles/resample_segments.txt]

Beside the time: the launches per call, the input read once plus the output written as bytes per second against the HBM peak
(8 TB/s; what the copy is held to), and the double FMAs the taps ask for -- two per tap here, the weight's and the sum's -- per
second against the FP64 vector peak (78.6 TFLOP/s = 39.3 T FMA/s).  The lines are printed and written to `--out`."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=100)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'resample_segments.txt'))
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = importlib.import_module('single-speaker-tts_amd._hip')
HBM_PEAK, FMA_PEAK, NWIN = 8.0e12, 39.3e12, 32769
UP4, DOWN3 = 2.0 ** (-4.0 / 12.0), 2.0 ** (3.0 / 12.0)

B, n = args.batch, args.samples
eng = sstts.Engine()
row = np.random.default_rng(0).standard_normal(n).astype(np.float32)
x = eng.empty((B, n))
for b in range(B):   # (filled row by row: one row of host random numbers)
    eng._check(eng.lib.tts_memcpy_h2d(eng.handle, x.ptr + b * row.nbytes, np.roll(row, 37 * b).ctypes.data, row.nbytes))
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def taps_of(ratio):
    """double FMAs per output sample: both wings' taps (off spread evenly), two FMAs a tap"""
    return 0.0 if ratio == 1.0 else 2.0 * 2.0 * (NWIN / int(min(1.0, ratio) * 512))


def timed(what, enqueue, outputs, fmas, launches_of=1.0):
    for rep in range(2):
        for _ in range(3):
            enqueue()
        eng.profile_reset()
        for _ in range(args.calls):
            enqueue()
        ms, launches = eng.profile_get('resample')
        s = ms * 1e-3 / args.calls * launches_of
        io = 4.0 * (B * n + outputs)
        say('    {:<44s} run {}: {:8.4f} ms per call, {:5.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak, {:6.2f} T FMA/s = {:5.2f} % of the '
            'FP64 vector peak, {:6.3f} ns per output sample'.format(what, rep, s * 1e3, launches / args.calls * launches_of, io / s / 1e9,
                                                                    100.0 * io / s / HBM_PEAK, fmas / s / 1e12, 100.0 * fmas / s / FMA_PEAK,
                                                                    s * 1e9 / max(outputs, 1)))
    return s


def segments_case(what, per_row):
    """per_row: (first, samples, ratio) of one row, repeated for every row"""
    seg = H.resample_segment_records([(b, f, c, r) for b in range(B) for f, c, r in per_row])
    counts = [H.resample_segment_count(c, r) for _f, c, r in per_row]
    N_out = max(sum(counts), 1)
    out = eng.empty((B, N_out))
    fmas = B * sum(c * taps_of(r) for c, (_f, _c, r) in zip(counts, per_row))
    s = timed(what, lambda: eng._check(eng.lib.tts_resample_segments(eng.handle, x.ptr, B, n, None, seg.ctypes.data, len(seg), N_out, out.ptr, None)),
              B * N_out, fmas)
    out.free()
    return s


def cut(k, ratios):
    """k segments that tile a row, ratios in turn"""
    edges = [n * i // k for i in range(k + 1)]
    return [(edges[i], edges[i + 1] - edges[i], ratios[i % len(ratios)]) for i in range(k)]


eng.set_option('profile', 1)
say('    {} x {} float32'.format(B, n))
segments_case('segments, all-copy (1 per row at 1.0)', cut(1, [1.0]))
one = segments_case('segments, 1 per row at 2 ** (-4 / 12)', cut(1, [UP4]))
N_out = H.resampled_length(n, UP4)
out = eng.empty((B, N_out))
fmas8 = N_out * taps_of(UP4) / 2.0 * (B + -(-B // 8))   # the sum's FMA per row, the weight's once per group of eight
batched = timed('tts_resample, batched (B = {})'.format(B), lambda: eng._check(eng.lib.tts_resample(eng.handle, x.ptr, B, n, None, UP4, N_out, out.ptr)),
                B * N_out, fmas8)
single = timed('tts_resample, B = 1 form, times {}'.format(B), lambda: eng._check(eng.lib.tts_resample(eng.handle, x.ptr, 1, n, None, UP4, N_out, out.ptr)),
               B * N_out, B * N_out * taps_of(UP4), launches_of=float(B))
out.free()
say('    one segment per row costs {:.2f} x the batched tts_resample and {:.2f} x its B = 1 form per sample'.format(one / batched, one / single))
segments_case('segments, 4 per row, mixed ratios', cut(4, [1.0, UP4, DOWN3, 0.5]))
segments_case('segments, 16 per row, mixed ratios', cut(16, [1.0, UP4, DOWN3, 0.5]))
eng.set_option('profile', 0)
x.free()
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
