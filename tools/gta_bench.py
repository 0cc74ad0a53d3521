#!/usr/bin/env python3
"""Teacher-forced decoder benchmark (tts_decoder_forward_teacher, reference tacotron/helpers.py:208-405): ms per call of 200
steps at T_s = 150 for B = 1, 32, 64, in both forms -- launch per layer (decoder.hip, never graph-captured) and the
weight-stationary kernel's teacher variant with 16 utterances per cluster (decoder_ws.hip, its pre-net inputs one GEMM in
front of the loop) -- next to the free-running call of the same form (tts_decoder_forward, the library's default options:
no hipGraph).  Device-resident inputs and outputs; wall clock over --iters calls after one warm-up call, the median of
--reps such runs.

    python tools/gta_bench.py [--iters 10] [--reps 3] [--out FILE]

Prints one line per (B, form) and one JSON line (also written to --out)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sstts = importlib.import_module('single-speaker-tts_amd')
W = importlib.import_module('single-speaker-tts_amd.tacotron.weights')
P = importlib.import_module('single-speaker-tts_amd.tacotron.params')

FORMS = {'launch_per_layer': (0, 0), 'ws16': (1, 16)}   # (persistent_decoder, rows per cluster)


def timed(eng, fn, iters, reps):
    fn()
    eng.synchronize()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        eng.synchronize()
        runs.append((time.perf_counter() - t0) / iters * 1e3)
    return float(np.median(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--Ts', type=int, default=150)
    ap.add_argument('--S', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    hp = P.ModelParams()
    eng = sstts.Engine(hp)
    eng.load_weights(W.synthetic_weights(0, hp))
    eng.set_option('debug_hooks', 1)
    rng = np.random.default_rng(0)
    res = dict(Ts=a.Ts, S=a.S, iters=a.iters, reps=a.reps, ms={})
    try:
        for B in (1, 32, 64):
            mem = eng.to_device((rng.standard_normal((B, a.Ts, 256)) * 0.5).astype(np.float32))
            tgt = eng.to_device(rng.random((B, a.S, hp.reduction * hp.n_mels)).astype(np.float32))
            mel = eng.empty((B, a.S, hp.reduction * hp.n_mels))
            al = eng.empty((a.S, B, a.Ts))
            for name, (pd, rows) in FORMS.items():
                eng.set_option('persistent_decoder', pd)
                eng.set_option('pd_rows', rows)
                choice = eng.teacher_kernel_choice(B, a.Ts)
                t_teacher = timed(eng, lambda: eng.decoder_forward_teacher(mem, tgt, mel=mel, alignments=al), a.iters, a.reps)
                t_free = timed(eng, lambda: eng.decoder_forward(mem, a.S, mel=mel, alignments=al), a.iters, a.reps)
                res['ms']['B{}_{}'.format(B, name)] = dict(teacher=round(t_teacher, 3), free=round(t_free, 3), kernel=choice)
                print('B={:2d} {:16s} teacher-forced {:7.2f} ms   free-running {:7.2f} ms   (teacher kernel choice {})'.format(
                    B, name, t_teacher, t_free, choice), flush=True)
    finally:
        eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
