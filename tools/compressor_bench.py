#!/usr/bin/env python3
"""The compressor stage (tts_compress) on an MI355X at bench.py's shape: 64 utterances of 275 000 samples at
22 050 Hz through the 'speech' profile, in place, apart, with the envelope written and with the records.  Device time per call from
profile stage "compress" over `--calls` calls after three warm-up calls, twice each.  Beside it, on the same rows: tts_equalize
through two sections (profile stage "equalize": the same cut, a linear recurrence, no transcendental function) and tts_limit at a
look-ahead of 110 samples with 4x oversampling (profile stage "limiter").

    python tools/compressor_bench.py [--calls 50] [--batch 64] [--samples 275000]

Beside the time: the bytes a call must move (the rows read three times and written once) per second and as a fraction of the HBM
peak (8 TB/s).  The input is restored before every timed block, so every block compresses the same rows."""
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
env = eng.empty((B, n), np.float64)
stats = eng.empty((B, 2), np.float64)
eng.set_option('profile', 1)
segs = -(-n // 256)
tiles = -(-n // 16384)
print('B = {}, n = {}: {} segments = {} waves of 64 per pass ({} tiles per utterance), 65 792 bytes of LDS per workgroup: two per compute unit'.format(
    B, n, B * segs, B * tiles, tiles))
params = H.TtsCompressor(*H.compressor_params(('profile', 'speech'), SR))
p_params = ctypes.addressof(params)
unity = H.TtsCompressor(*H.compressor_params(('design', (-18.0, 1.0, 6.0, 5.0, 100.0, 0.0)), SR))
sos = np.ascontiguousarray(H.equalizer_profile('warm', SR))
p_sos = sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def timed(name, stage, call, nbytes):
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
        print('{:28s} run {}: {:8.4f} ms per call, {:4.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            name, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)


rows = 4.0 * B * n
lib, h = eng.lib, eng.handle
# (in place the rows change from call to call -- a compressed row is compressed again -- so the apart form is the steady one)
timed('compress, apart', 'compress', lambda: lib.tts_compress(h, x.ptr, y.ptr, B, n, None, p_params, None, None), 4.0 * rows)
timed('compress, in place', 'compress', lambda: lib.tts_compress(h, x.ptr, x.ptr, B, n, None, p_params, None, None), 4.0 * rows)
timed('compress, ratio 1 (identity)', 'compress', lambda: lib.tts_compress(h, x.ptr, y.ptr, B, n, None, ctypes.addressof(unity), None, None), 4.0 * rows)
timed('compress, with envelope', 'compress', lambda: lib.tts_compress(h, x.ptr, y.ptr, B, n, None, p_params, env.ptr, None), 6.0 * rows)
timed('compress, with records', 'compress', lambda: lib.tts_compress(h, x.ptr, y.ptr, B, n, None, p_params, None, stats.ptr), 4.0 * rows)
timed('equalize, S = 2, apart', 'equalize', lambda: lib.tts_equalize(h, x.ptr, y.ptr, B, n, None, p_sos, 2), 3.0 * rows)
timed('limit, L = 110, 4x', 'limiter', lambda: lib.tts_limit(h, x.ptr, B, n, None, 0.25, 110, 4, stats.ptr), 3.0 * rows)
