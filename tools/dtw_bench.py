#!/usr/bin/env python3
"""Mel-cepstral distortion on an MI355X: the cepstra (tts_mfcc) and the alignment (tts_dtw) of audio.metrics, stage by stage.

    python tools/dtw_bench.py [--reps 20] [--warmup 3]

Device times per call from the library's own HIP events (profile stages "mfcc" and "dtw"), after warm-up calls that also grow the
workspaces.  Lines:
  (a) tts_mfcc, 64 x 1000 rows of 80 mel bands -> 14 coefficients, clipped, and at B = 1;
  (b) tts_dtw at 64 pairs of 1000 x 1000 frames, D = 13 in the ptr + 1 form on those coefficients, with and without a path, and at
      B = 1;
  (c) what bounds the kernel: the same call at other lengths, batch sizes and frame widths -- a workgroup per pair walks
      na + nb - 1 anti-diagonals with a barrier behind each, so the time per diagonal is the figure to read: it does not move with
      B while the pairs have a compute unit each, it moves with the slots of rows a lane owns (ceil(na / tts_dtw_tile())) and
      with D (the local cost of a cell is 2 D loads and 3 D double operations of one lane)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
eng = sstts.Engine()
TILE = eng.dtw_tile()
rng = np.random.default_rng(0)


def timed(stage, call):
    for _ in range(args.warmup):
        eng._check(call())
    eng.set_option('profile', 1)
    eng.profile_reset()
    for _ in range(args.reps):
        eng._check(call())
    ms, launches = eng.profile_get(stage)
    eng.set_option('profile', 0)
    return ms / args.reps, launches // args.reps


def cepstra(B, T):
    """(B, T, 14) device cepstra of random-walk mel rows: neighbouring frames are alike, as in speech"""
    mel = np.clip(0.5 + np.cumsum(rng.standard_normal((B, T, 80)) * 0.02, axis=1), 0, 1).astype(np.float32)
    d_mel = eng.to_device(mel)
    out = eng.empty((B, T, 14))
    ms, launches = timed('mfcc', lambda: eng.lib.tts_mfcc(eng.handle, d_mel.ptr, B, T, 80, 80, None, 14, 1, out.ptr))
    d_mel.free()
    return out, ms, launches


def dtw(ca, cb, B, na, nb, D, skip, want_path):
    K = ca.shape[2]
    cost, plen = eng.empty((B,), np.float64), eng.empty((B,), np.int32)
    path = eng.empty((B, na + nb - 1, 2), np.int32) if want_path else None
    ms, launches = timed('dtw', lambda: eng.lib.tts_dtw(eng.handle, ca.ptr + 4 * skip, na, K, None, cb.ptr + 4 * skip, nb, K, None, B, D,
                                                        cost.ptr, plen.ptr, path.ptr if want_path else None))
    mean_len = float(plen.to_host().mean())
    for x in (cost, plen, path):
        if x is not None:
            x.free()
    return ms, launches, mean_len


def line(tag, B, na, nb, D, ms, launches, mean_len, want_path):
    diags = na + nb - 1
    print('{} tts_dtw B = {:3d}, {} x {} frames, D = {:3d}, {}: {:8.3f} ms per call ({} launch{}), {} diagonals -> {:6.0f} ns per '
          'diagonal, {:.2f} G cells/s; mean path_len {:.0f}'.format(
              tag, B, na, nb, D, 'path   ' if want_path else 'no path', ms, launches, '' if launches == 1 else 'es', diags, ms * 1e6 / diags,
              B * na * nb / (ms * 1e6), mean_len), flush=True)


# ---- (a), (b): the flagship shape
for B in (64, 1):
    ca, ms_a, la = cepstra(B, 1000)
    cb, ms_b, lb = cepstra(B, 1000)
    print('(a) tts_mfcc B = {:3d}, 1000 x 80 -> 14, clip01: {:.1f} us per call ({} launch)'.format(B, 0.5 * (ms_a + ms_b) * 1e3, la), flush=True)
    for want_path in (False, True):
        line('(b)', B, 1000, 1000, 13, *dtw(ca, cb, B, 1000, 1000, 13, 1, want_path), want_path)
    ca.free()
    cb.free()

# ---- (c): what the time follows
print('(c) tile = {} rows per slot, {} frames at most'.format(TILE, eng.dtw_max_frames()), flush=True)
for B, na, nb in ((64, 250, 250), (64, 500, 500), (64, 512, 1488), (64, 1488, 512), (64, 2000, 2000), (16, 1000, 1000), (256, 1000, 1000), (1024, 1000, 1000)):
    ca, _, _ = cepstra(B, na)
    cb, _, _ = cepstra(B, nb)
    line('(c)', B, na, nb, 13, *dtw(ca, cb, B, na, nb, 13, 1, False), False)
    ca.free()
    cb.free()
for D in (1, 4, 16, 17, 64, 128):
    x = eng.to_device(np.cumsum(rng.standard_normal((64, 1000, D)), axis=1).astype(np.float32))
    y = eng.to_device(np.cumsum(rng.standard_normal((64, 1000, D)), axis=1).astype(np.float32))
    line('(c)', 64, 1000, 1000, D, *dtw(x, y, 64, 1000, 1000, D, 0, False), False)
    x.free()
    y.free()
eng.close()
