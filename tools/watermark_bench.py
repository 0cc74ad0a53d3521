#!/usr/bin/env python3
"""The watermark stages (tts_watermark_embed, tts_watermark_detect) on an MI355X at bench.py's shape: 64 utterances
of 275 000 samples, the default carrier (16 bits, 8 samples a chip, 64 chips a symbol).  Device time per call from profile stage
"watermark" over `--calls` calls after three warm-up calls, twice each: the embedder apart, in place and with the records, the
detector at 64 and at 1024 offsets.  Beside the embedder, on the same rows: tts_encode to 16-bit PCM without dither (profile stage
"encode"), the other one-pass streaming stage.

    python tools/watermark_bench.py [--calls 50] [--batch 64] [--samples 275000]

Beside the time: for the embedder the bytes a call must move (the rows read twice and written once) per second and as a fraction of
the HBM peak (8 TB/s); for the detector the N D / L multiply-adds of the correlation per second."""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=50)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = sstts._hip
HBM_PEAK = 8.0e12
SR = 22050

B, n = args.batch, args.samples
eng = sstts.Engine()
rng = np.random.default_rng(0)
row = (0.3 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(np.arange(n) * (2.0 * np.pi * 3.1 / SR)))).astype(np.float32)
host = np.stack([np.roll(row, 37 * b) for b in range(B)])
x = eng.to_device(host)
y = eng.empty((B, n))
codes = eng.empty((B, n), np.int16)
stats = eng.empty((B, 2), np.float64)
records = eng.empty((B, 4), np.float64)
eng.set_option('profile', 1)
params = H.TtsWatermark(*H.watermark_setting((0x5EED, 0xA5C3)))
p_params = ctypes.addressof(params)
L = params.chip
print('B = {}, n = {}: {} tiles of 4096 samples per utterance, {} chips of {} samples per phase'.format(B, n, -(-n // 4096), (n + 2 * L - 2) // L, L))


def timed(name, stage, call, nbytes=None, macs=None):
    for rep in range(2):
        x.copy_from(host)
        for _ in range(3):
            eng._check(call())
        x.copy_from(host)
        eng.profile_reset()
        for _ in range(args.calls):
            eng._check(call())
        ms, launches = eng.profile_get(stage)
        per = ms / args.calls
        rate = '{:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK) if nbytes else \
            '{:7.1f} G multiply-adds per second'.format(macs / per / 1e6)
        print('{:28s} run {}: {:8.4f} ms per call, {:4.1f} launches, {}'.format(name, rep, per, launches / args.calls, rate), flush=True)


rows = 4.0 * B * n
lib, h = eng.lib, eng.handle
# (in place the rows change from call to call -- a marked row is marked again -- so the apart form is the steady one)
timed('embed, apart', 'watermark', lambda: lib.tts_watermark_embed(h, x.ptr, y.ptr, B, n, None, p_params, None), nbytes=3.0 * rows)
timed('embed, in place', 'watermark', lambda: lib.tts_watermark_embed(h, x.ptr, x.ptr, B, n, None, p_params, None), nbytes=3.0 * rows)
timed('embed, with records', 'watermark', lambda: lib.tts_watermark_embed(h, x.ptr, y.ptr, B, n, None, p_params, stats.ptr), nbytes=3.0 * rows)
timed('encode, pcm16, no dither', 'encode', lambda: lib.tts_encode(h, x.ptr, B, n, None, H.FMT_PCM_S16, 0, 0, codes.ptr, stats.ptr), nbytes=1.5 * rows)
for D in (64, 1024):
    timed('detect, D = {}'.format(D), 'watermark', lambda: lib.tts_watermark_detect(h, x.ptr, B, n, None, p_params, D, records.ptr, None, None),
          macs=float(B) * n * D / L)
