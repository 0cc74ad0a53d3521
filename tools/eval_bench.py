#!/usr/bin/env python3
"""Mode.EVAL benchmark: ms per tts_evaluate batch of B = 32 at LJ-Speech-like lengths (T_sent = 150 ids, 160 reduced frames =
800 frames of 1025 bins), and the loss reduction alone (profile stage "eval_loss", device events): its time and its achieved
bandwidth against the HBM peak (8.0 TB/s spec, ~6.3 TB/s achievable: MI355X_MICROARCH.md).  Bytes are what the two launches must
move: both targets and both outputs read once, the chunk partials written and read back.

    python tools/eval_bench.py [--B 32] [--Ts 150] [--steps 160] [--iters 10] [--out FILE]

Prints one JSON line (and writes it to --out)."""
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

EL_CHUNK = 8192   # floats per chunk of csrc/eval_loss.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--Ts', type=int, default=150)
    ap.add_argument('--steps', type=int, default=160)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    hp = P.ModelParams()
    eng = sstts.Engine(hp)
    eng.load_weights(W.synthetic_weights(0, hp))
    rng = np.random.default_rng(0)
    B, Ts, S = a.B, a.Ts, a.steps
    r, nm, F = hp.reduction, hp.n_mels, 1 + hp.n_fft // 2
    T = S * r
    ids = np.zeros((B, Ts), np.int32)
    for b in range(B):   # uneven sentence lengths, padded with 0 as the batcher pads them
        L = int(rng.integers(Ts * 2 // 3, Ts))
        ids[b, :L - 1] = rng.integers(2, 39, L - 1)
        ids[b, L - 1] = 1
    mel_t = eng.to_device(rng.random((B, S, r * nm)).astype(np.float32))
    lin_t = eng.to_device(rng.random((B, S, r * F)).astype(np.float32))
    d_ids = eng.to_device(ids)
    losses = eng.empty((3,))
    for _ in range(2):   # warm-up: code objects, workspaces
        eng.evaluate(d_ids, mel_t, lin_t, losses=losses)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        eng.evaluate(d_ids, mel_t, lin_t, losses=losses)
    eng.synchronize()
    ms_batch = (time.perf_counter() - t0) * 1e3 / a.iters
    eng.set_option('profile', 1)
    eng.profile_reset()
    for _ in range(a.iters):
        eng.evaluate(d_ids, mel_t, lin_t, losses=losses)
    stages = {}
    for st in ('encoder', 'decoder', 'postnet', 'eval_loss'):
        ms, n = eng.profile_get(st)
        stages[st] = ms / a.iters
    eng.set_option('profile', 0)
    n_el = B * T * (nm + F)
    n_partial = B * (-(-(T * nm + 3) // EL_CHUNK) + -(-(T * F + 3) // EL_CHUNK))
    bytes_loss = 2 * 4 * n_el + 2 * 8 * n_partial + 16 * B
    loss_ms = stages['eval_loss']
    res = dict(bench='eval', B=B, T_sent=Ts, n_steps=S, frames=T, ms_per_batch=round(ms_batch, 3),
               stage_ms={k: round(v, 4) for k, v in stages.items()}, loss_bytes=bytes_loss,
               loss_TBps=round(bytes_loss / (loss_ms * 1e-3) / 1e12, 3) if loss_ms > 0 else None,
               loss_share_of_hbm_spec=round(bytes_loss / (loss_ms * 1e-3) / 8.0e12, 3) if loss_ms > 0 else None,
               loss_share_of_batch=round(loss_ms / ms_batch, 4), losses=[float(x) for x in losses.to_host()],
               device=eng.device_info()[1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    eng.close()


if __name__ == '__main__':
    main()
