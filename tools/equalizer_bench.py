#!/usr/bin/env python3
"""The equaliser stage (tts_equalize) on an MI355X at bench.py's shape: 64 utterances of 275 000 samples at 22 050 Hz
through cascades of 1, 4 and 8 sections, in place.  Device time per call from profile stage "equalize" over `--calls` calls after
three warm-up calls, twice each.  Beside it, on the same buffers: tts_loudness_normalize (profile stage "loudness": the same
recurrence for one fixed pair of sections, read straight from memory, nothing written but a gain pass) and a device-to-device copy
of the rows (hipMemcpyAsync, timed by the host clock around `--calls` copies and one synchronisation: the bytes' own time).

    python tools/equalizer_bench.py [--calls 50] [--batch 64] [--samples 275000]

Beside the time: the bytes a call must move (the rows read twice and written once, the states written and read twice) per second
and as a fraction of the HBM peak (8 TB/s), the double operations of the two passes per second (9 per sample, section and pass),
and the waves the cut makes against the two that fit a compute unit's LDS."""
import argparse
import ctypes
import importlib
import os
import sys
import time

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
row = (0.1 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(np.arange(n) * (2.0 * np.pi * 3.1 / SR)))).astype(np.float32)
host = np.stack([np.roll(row, 37 * b) for b in range(B)])
x = eng.to_device(host)
y = eng.empty((B, n))
eng.set_option('profile', 1)
pool = np.concatenate([H.equalizer_profile('telephony', SR), H.equalizer_profile('warm', SR), H.equalizer_profile('small-speaker', SR)[2:],
                       H.equalizer_profile('bright', SR)])
segs = -(-n // 256)
tiles = -(-n // 16384)
print('B = {}, n = {}: {} segments = {} waves of 64 per pass ({} tiles per utterance), 65 792 bytes of LDS per workgroup: two per compute unit'.format(
    B, n, B * segs, B * tiles, tiles))


def timed(name, stage, call, nbytes, flops=0.0):
    for rep in range(2):
        for _ in range(3):
            eng._check(call())
        eng.profile_reset()
        for _ in range(args.calls):
            eng._check(call())
        ms, launches = eng.profile_get(stage)
        per = ms / args.calls
        line = '{:22s} run {}: {:8.4f} ms per call, {:4.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
            name, rep, per, launches / args.calls, nbytes / per / 1e6, 100.0 * nbytes / (per * 1e-3) / HBM_PEAK)
        if flops:
            line += ', {:6.2f} TFLOP/s in double'.format(flops / (per * 1e-3) / 1e12)
        print(line, flush=True)


rows = 4.0 * B * n
for S in (1, 4, 8):
    sos = np.ascontiguousarray(pool[:S])
    p_sos = sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    states = 8.0 * B * segs * 2 * S
    timed('equalize, S = %d' % S, 'equalize', lambda: eng.lib.tts_equalize(eng.handle, x.ptr, x.ptr, B, n, None, p_sos, S), 3.0 * rows + 4.0 * states,
          flops=2.0 * 9.0 * S * B * n)
    x.copy_from(host)
timed('equalize, S = 4, apart', 'equalize', lambda: eng.lib.tts_equalize(eng.handle, x.ptr, y.ptr, B, n, None, p_sos, 4), 3.0 * rows)
timed('loudness_normalize', 'loudness', lambda: eng.lib.tts_loudness_normalize(eng.handle, x.ptr, B, n, None, SR, -23.0, 1.0, None, None), 5.0 * rows)

hip = ctypes.CDLL('libamdhip64.so')
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
eng.synchronize()
for rep in range(2):
    for k in range(3 + args.calls):
        if k == 3:
            assert hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(y.ptr, x.ptr, int(rows), 3, None) == 0          # 3: device to device
    assert hip.hipDeviceSynchronize() == 0
    per = (time.perf_counter() - t0) * 1e3 / args.calls
    print('{:22s} run {}: {:8.4f} ms per call (host clock), {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
        'device-to-device copy', rep, per, 2.0 * rows / per / 1e6, 100.0 * 2.0 * rows / (per * 1e-3) / HBM_PEAK))
