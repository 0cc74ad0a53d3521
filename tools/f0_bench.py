#!/usr/bin/env python3
"""F0 tracking on an MI355X: tts_f0 (YIN, csrc/f0.hip) and tts_f0_compare of audio.metrics, profile stage "f0".

    python tools/f0_bench.py [--reps 10] [--warmup 2] [--out profiles/f0.txt]

Device times per call from the library's own HIP events, after warm-up calls.  Lines:
  (a) tts_f0 at 64 x 275 000 samples (12.5 s at 22050 Hz), hop 275, W 1024, lags 44 .. 368, and at B = 1;
  (b) tts_f0_compare at 64 pairs along diagonal paths of 1001 x 1001 frames;
  (c) what bounds the kernel.  The definition fixes 3 W tau_max double operations per frame (a difference, a product and a sum per
      lag and j, none fused), and the kernel reads (slots + 1) doubles from LDS per j and lane -- one broadcast x(s0 + j) and one
      x(s0 + j + tau) per slot of 256 lags.  The same call at other lag counts separates the two: at tau_max = 256, 512, 768 and
      1024 every lane slot is busy, so a double-issue bound keeps the time per (lag, j) pair level while an LDS-read bound lets it
      fall as (slots + 1) / slots = 2, 1.5, 1.33, 1.25; tau_max = 368 leaves 28 % of the second slot idle.  Other W and hop move
      the share of the staging, the normalisation chain and the decisions.
With --out the lines are also written to that file."""
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
SR = 22050.0
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
    ms, launches = eng.profile_get('f0')
    eng.set_option('profile', 0)
    return ms / args.reps, launches // args.reps


def speech_like(B, N):
    """harmonic tones with a slow vibrato and some noise: voiced frames that take the whole decision path"""
    t = np.arange(N, dtype=np.float64) / SR
    x = np.zeros((B, N), np.float32)
    for b in range(B):
        f = 90.0 + 8.0 * (b % 32) + 6.0 * np.sin(2 * np.pi * 3.0 * t + b)
        ph = 2 * np.pi * np.cumsum(f) / SR
        x[b] = (0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + 0.1 * np.sin(3 * ph + 2.0) + 0.02 * rng.standard_normal(N)).astype(np.float32)
    return x


def f0(tag, d_x, B, N, hop, W, lo, hi):
    T = 1 + N // hop
    out, apd = eng.empty((B, T)), eng.empty((B, T))
    ms, launches = timed(lambda: eng.lib.tts_f0(eng.handle, d_x.ptr, B, N, None, SR, hop, W, lo, hi, 0.1, out.ptr, apd.ptr))
    voiced = float((out.to_host() > 0).mean())
    out.free()
    apd.free()
    frames = B * T
    ops = 3.0 * W * hi * frames
    slots = -(-hi // 256)
    lds = 8.0 * (slots + 1) * W * 256 * frames
    say('{} tts_f0 B = {:3d}, {} samples, hop {}, W {}, lags {} .. {}: {:9.3f} ms per call ({} launch{}), {} frames -> {:7.2f} us per '
        'frame, {:6.2f} T double op/s, {:6.2f} TB/s of LDS reads, {:6.3f} ps per (lag, j) pair; {:.2f} voiced'.format(
            tag, B, N, hop, W, lo, hi, ms, launches, '' if launches == 1 else 'es', frames, ms * 1e3 / frames, ops / (ms * 1e9),
            lds / (ms * 1e9), ms * 1e9 / (W * hi * frames), voiced))


say('tts_f0: 3 W tau_max double operations per frame by definition; peak separate double adds / products of the chip: '
    '256 CUs x 64 lanes / 4 cycles x 2.4 GHz = 39 T op/s; LDS reads of 8 bytes: about 150 TB/s')
# ---- (a): the flagship shape
N = 275000
x64 = speech_like(64, N)
d64 = eng.to_device(x64)
f0('(a)', d64, 64, N, 275, 1024, 44, 368)
f0('(a)', d64, 1, N, 275, 1024, 44, 368)

# ---- (b): the comparison
T = 1 + N // 275
tracks = eng.f0(d64, SR, 275)
path = np.full((64, 2 * T - 1, 2), -1, np.int32)
path[:, :T, 0] = path[:, :T, 1] = np.arange(T)
d_path = eng.to_device(path)
counts, sums = eng.empty((64, 5), np.int32), eng.empty((64, 2), np.float64)
half = 32 * T * 4
ms, launches = timed(lambda: eng.lib.tts_f0_compare(eng.handle, tracks.ptr, T, tracks.ptr + half, T, d_path.ptr, 2 * T - 1, 32, counts.ptr, sums.ptr))
say('(b) tts_f0_compare B = 32, {} x {} frames, {} path rows: {:.1f} us per call ({} launch)'.format(T, T, 2 * T - 1, ms * 1e3, launches))
for d in (tracks, d_path, counts, sums):
    d.free()

# ---- (c): what the time follows
for hi in (256, 512, 768, 1024):
    f0('(c)', d64, 64, N, 275, 1024, 44, hi)
for W in (256, 2048):
    f0('(c)', d64, 64, N, 275, W, 44, 368)
for hop in (128, 1024):
    f0('(c)', d64, 64, N, hop, 1024, 44, 368)
for B in (8, 16):
    f0('(c)', d64, B, N, 275, 1024, 44, 368)
d64.free()
eng.close()
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
