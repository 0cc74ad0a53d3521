#!/usr/bin/env python3
"""STOI / ESTOI on an MI355X: tts_stoi (csrc/stoi.hip) behind audio.metrics.stoi, profile stage "stoi".

    python tools/stoi_bench.py [--reps 10] [--warmup 2] [--out profiles/stoi.txt]

Device times per call from the library's own HIP events, after warm-up calls.  Lines:
  (a) tts_stoi at 64 rows x 124 717 samples -- 275 000 samples at 22 050 Hz brought to 10 kHz -- in both modes, with the
      workspaces of the call and with the caller's index and envelope buffers, and at B = 1;
  (b) the same call on rows of which half the frames are silent: the envelope and segment launches follow the kept frames.
The times of the five launches come from a kernel trace of this program:
    rocprofv3 --kernel-trace --stats -- python tools/stoi_bench.py --reps 5
(profiles/stoi.txt has one).  With --out the lines are also written to that file."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--out', default=None)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
eng = sstts.Engine()
rng = np.random.default_rng(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(call):
    for _ in range(args.warmup):
        eng._check(call())
    eng.set_option('profile', 1)
    eng.profile_reset()
    for _ in range(args.reps):
        eng._check(call())
    ms, launches = eng.profile_get('stoi')
    eng.set_option('profile', 0)
    return ms / args.reps, launches // args.reps


def rows(B, N, gated):
    """noise under a slow envelope; ``gated``: bursts with silence between them (about half the frames are dropped)"""
    t = np.arange(N) / 10000.0
    x = np.zeros((B, N), np.float32)
    for b in range(B):
        env = 0.3 + 0.7 * np.abs(np.sin(2 * np.pi * (0.37 + 0.01 * b) * t))
        if gated:
            env = env * np.clip(np.sin(2 * np.pi * 3.1 * t + b), 0, None) ** 2
        x[b] = (0.2 * env * rng.standard_normal(N)).astype(np.float32)
    return x


def stoi(tag, d_ref, d_deg, B, N, extended, own):
    cap = eng.lib.tts_stoi_frames(N)
    rec = eng.empty((B, 3), np.float64)
    idx = eng.empty((B, cap), np.int32) if own else None
    env = eng.empty((B, 2, 15, cap), np.float64) if own else None
    ms, launches = timed(lambda: eng.lib.tts_stoi(eng.handle, d_ref.ptr, d_deg.ptr, B, N, None, int(extended), rec.ptr,
                                                  idx.ptr if own else None, env.ptr if own else None))
    r = rec.to_host().view(sstts._hip.STOI_RECORD).reshape(B)
    for a in (rec, idx, env):
        if a is not None:
            a.free()
    frames, kept = int(r['frames'].sum()), int(r['kept'].sum())
    say('{} tts_stoi B = {:3d}, {} samples, {}, {} buffers: {:8.3f} ms per call ({} launches), {} frames, {} kept, {} segments -> '
        '{:6.3f} us per kept frame (two real transforms of 512 points each); mean value {:.4f}'.format(
            tag, B, N, 'ESTOI' if extended else 'STOI ', "the caller's" if own else "the call's own", ms, launches, frames, kept,
            int(r['segments'].sum()), ms * 1e3 / max(kept, 1), float(np.nanmean(r['value']))))


N = 124717
say('tts_stoi: per kept frame two 256-point complex double transforms in LDS (8 stages of 64 radix-4 butterflies) and 2 x 212 bins '
    'unfolded and summed; per segment 15 x 30 envelope pairs')
for gated, tag in ((False, '(a)'), (True, '(b)')):
    ref = rows(64, N, gated)
    deg = (ref + 0.05 * rng.standard_normal(ref.shape)).astype(np.float32)
    d_ref, d_deg = eng.to_device(ref), eng.to_device(deg)
    for extended in (False, True):
        stoi(tag, d_ref, d_deg, 64, N, extended, False)
        stoi(tag, d_ref, d_deg, 64, N, extended, True)
    stoi(tag, d_ref, d_deg, 1, N, False, False)
    d_ref.free()
    d_deg.free()
eng.close()
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
