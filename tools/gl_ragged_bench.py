#!/usr/bin/env python3
"""The ragged Griffin-Lim call (tts_griffin_lim_ragged) against what a caller had before it: B = 64 utterances whose lengths
are spread evenly over 300 ... 1000 frames, 1102 / 275, 60 iterations, explicit initial phases, ms per call from device-side
completion (a host clock around calls that end in a synchronise; five calls after a warm-up call).

    python tools/gl_ragged_bench.py [--iters 60] [--reps 5] [--momentum 0.99] [--uniform-only]
    python tools/gl_ragged_bench.py --reconstruction [--files 64] [--iters 60]

Lines: (a) the uniform call on the batch padded to T_max, the only batched form without the ragged call; (b) that time scaled
by sum(T_b) / (B T_max), what the frames alone would cost; the ragged call, its distance from (b), and the two terms the cut
accounts for -- 11 frames per run and the edge path of 2 halo frames per utterance; one call per utterance (B = 1) for
comparison.  ``--uniform-only`` times (a) alone: run it with SSTTS_HIP_LIB set to another build of the library for a same-box
A/B of the default path.  ``--reconstruction``: datasets.statistics.collect_reconstruction_error on generated WAV files of
1 ... 10 s at 22.05 kHz, files per second, analysis and host packing included."""
import argparse
import ctypes
import importlib
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=60)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--momentum', type=float, default=0.0)
ap.add_argument('--uniform-only', action='store_true')
ap.add_argument('--reconstruction', action='store_true')
ap.add_argument('--files', type=int, default=64)
args = ap.parse_args()
sstts = importlib.import_module('single-speaker-tts_amd')
eng = sstts.Engine()
if args.momentum:
    eng.set_option('gl_momentum', sstts._hip.momentum_thousandths(args.momentum))
N_FFT, WIN, HOP, F = 2048, 1102, 275, 1025


def timed(call, reps):
    call()
    eng.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        eng.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def fmt(ms):
    return ' '.join('{:.3f}'.format(m) for m in ms) + ' ms per call, min {:.3f}'.format(min(ms))


if args.reconstruction:
    ST = importlib.import_module('single-speaker-tts_amd.datasets.statistics')
    io = importlib.import_module('single-speaker-tts_amd.audio.io')
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        paths, seconds = [], 0.0
        for k in range(args.files):
            n = int(rng.uniform(1.0, 10.0) * 22050)
            t = np.arange(n) / 22050.0
            io.save_wav(os.path.join(d, '{}.wav'.format(k)), (0.3 * np.sin(2 * np.pi * (200 + 5 * k) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32), 22050)
            paths.append(os.path.join(d, '{}.wav'.format(k)))
            seconds += n / 22050.0
        ST.collect_reconstruction_error(paths[:4], 2, engine=eng, seed=1)   # warm-up
        eng.synchronize()
        t0 = time.perf_counter()
        ST.collect_reconstruction_error(paths, args.iters, batch_size=32, engine=eng, seed=1)
        eng.synchronize()
        dt = time.perf_counter() - t0
    print('reconstruction error: {} files ({:.0f} s of audio), {} iterations: {:.2f} s, {:.1f} files/s, {:.0f} x real time'.format(
        args.files, seconds, args.iters, dt, args.files / dt, seconds / dt))
    sys.exit(0)

B, T_MAX = 64, 1000
lengths = [int(round(v)) for v in np.linspace(300, T_MAX, B)]
rng = np.random.default_rng(0)
mag_h = (rng.random((B, F, T_MAX), dtype=np.float32) ** 4) * 10
init_h = rng.random((B, F, T_MAX), dtype=np.float32)
mag, init = eng.to_device(mag_h), eng.to_device(init_h)
uni = timed(lambda: eng.griffin_lim(mag, args.iters, WIN, HOP, N_FFT, init_phase=init, want_mse=False), args.reps)
print('(a) uniform, padded to {}: {}'.format(T_MAX, fmt(uni)), flush=True)
if args.uniform_only:
    sys.exit(0)
share = sum(lengths) / float(B * T_MAX)
a = min(uni)
print('(b) frames alone: sum T_b / (B T_max) = {:.4f} of (a) = {:.3f} ms'.format(share, a * share))
rag = timed(lambda: eng.griffin_lim(mag, args.iters, WIN, HOP, N_FFT, init_phase=init, want_mse=False, n_frames=lengths), args.reps)
print('ragged call: {}'.format(fmt(rag)), flush=True)
# what the cut accounts for, in frames: 11 per run (both plans, from the host-only planner on this chip's compute units),
# and the edge path of 2 halo frames per utterance, which costs a frame's worth more than an interior frame at most
lib = eng.lib
n_cus = ctypes.c_int(0)
uuid = ctypes.create_string_buffer(33)
lib.tts_device_info(eng.handle, uuid, ctypes.byref(n_cus))
cap = 65536
buf = (ctypes.c_int * (4 * cap))()
nf = np.asarray(lengths, np.int32)
runs_r = lib.tts_debug_gl_plan_ragged(nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B, WIN, HOP, n_cus.value, buf, cap, None)
runs_u = lib.tts_debug_gl_plan(T_MAX, B, WIN, HOP, n_cus.value, buf, cap, None)
halo = -(-WIN // HOP) - 1
work_u = B * T_MAX + 11 * runs_u
work_r = sum(lengths) + 11 * runs_r
print('runs: uniform {} ragged {} on {} compute units; frames + 11 per run: ragged / uniform = {:.4f} -> {:.3f} ms expected; '
      'edge-path frames {} of {} ({:.2f} %)'.format(runs_u, runs_r, n_cus.value, work_r / work_u, a * work_r / work_u,
                                                     2 * halo * B, sum(lengths), 200.0 * halo * B / sum(lengths)))
print('distance from (b): {:+.3f} ms ({:+.1f} %); from the per-run model: {:+.3f} ms ({:+.1f} %)'.format(
    min(rag) - a * share, 100 * (min(rag) / (a * share) - 1), min(rag) - a * work_r / work_u, 100 * (min(rag) / (a * work_r / work_u) - 1)))
# one call per utterance: what a caller with different lengths had to do
mags = [eng.to_device(np.ascontiguousarray(mag_h[b:b + 1, :, :T])) for b, T in list(enumerate(lengths))[::8]]
inits = [eng.to_device(np.ascontiguousarray(init_h[b:b + 1, :, :T])) for b, T in list(enumerate(lengths))[::8]]


def one_by_one():
    for m, u in zip(mags, inits):
        eng.griffin_lim(m, args.iters, WIN, HOP, N_FFT, init_phase=u, want_mse=False)


per = timed(one_by_one, 2)
print('one call per utterance (every eighth utterance, times 8): {:.3f} ms for the batch'.format(min(per) * 8))
