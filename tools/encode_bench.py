#!/usr/bin/env python3
"""The delivery encoder (tts_encode) on an MI355X at bench.py's shape: 64 rows of 275 000 samples, every format,
with and without the TPDF dither.  Device time per call from profile stage "encode" over `--calls` calls after three warm-up
calls, twice each.  Beside the time: the bytes a call must move -- the float32 rows read once, the codes written once -- per
second and as a fraction of the HBM peak (8 TB/s).

    python tools/encode_bench.py [--calls 50] [--batch 64] [--samples 275000]

With `--stream` instead: the step of `tacotron.inference.synthesize_stream` at bench.py's shape (host ids in, three calls in
flight, what comes back read on the host) with the delivery format off, then 'pcm16', then mu-law at 8 kHz, `--steps` steps each
after `--warmup`, `--repeats` times round: what `bench.py --through-facade` times, with the setting switched.  The bytes each
answer carries across the host boundary are printed beside the time.

    python tools/encode_bench.py --stream [--steps 20] [--warmup 3] [--repeats 2]"""
import argparse
import importlib
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=50)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--samples', type=int, default=275000)
ap.add_argument('--stream', action='store_true')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--repeats', type=int, default=2)
args = ap.parse_args()

sstts = importlib.import_module('single-speaker-tts_amd')
H = sstts._hip
HBM_PEAK = 8.0e12


def stage():
    B, n = args.batch, args.samples
    eng = sstts.Engine()
    rng = np.random.default_rng(0)
    row = (0.25 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(np.arange(n) * (2.0 * np.pi * 3.1 / 22050)))).astype(np.float32)
    x = eng.to_device(np.stack([np.roll(row, 37 * b) for b in range(B)]))
    out = eng.empty((B, n), np.int16)
    stats = eng.empty((B, 4), np.int32)
    eng.set_option('profile', 1)
    print('B = {}, n = {}: {} tiles of {} samples per row'.format(B, n, -(-n // H.ENCODE_TILE), H.ENCODE_TILE))
    for name in ('pcm16', 'pcm8', 'mulaw', 'alaw'):
        fmt = H.FORMATS[name]
        nbytes = float(B) * n * (4 + eng.lib.tts_encode_width(fmt))
        for dither in (H.DITHER_NONE, H.DITHER_TPDF):
            call = lambda: eng.lib.tts_encode(eng.handle, x.ptr, B, n, None, fmt, dither, 1234, out.ptr, stats.ptr)
            for rep in range(2):
                for _ in range(3):
                    eng._check(call())
                eng.profile_reset()
                for _ in range(args.calls):
                    eng._check(call())
                ms, launches = eng.profile_get('encode')
                per = ms / args.calls
                print('{:6s} {:6s} run {}: {:8.4f} ms per call, {:3.1f} launches, {:7.1f} GB/s = {:5.2f} % of the HBM peak'.format(
                    name, 'tpdf' if dither else 'plain', rep, per, launches / args.calls, nbytes / per / 1e6,
                    100.0 * nbytes / (per * 1e-3) / HBM_PEAK), flush=True)
        st = stats.to_host().view(H.ENCODE_RECORD).reshape(B)
        print('    last call: {} of {} samples clipped, peak {}'.format(int(st['clipped'].sum()), B * n, int(st['peak'].max())))


def stream():
    import bench
    P = importlib.import_module('single-speaker-tts_amd.tacotron.params')
    Wm = importlib.import_module('single-speaker-tts_amd.tacotron.weights')
    Tm = importlib.import_module('single-speaker-tts_amd.tacotron.model')
    Inf = importlib.import_module('single-speaker-tts_amd.tacotron.inference')
    hp = P.ModelParams()
    eng = sstts.Engine(hp)
    eng.load_weights_blob(Wm.pack_blob(Wm.synthetic_weights(0, hp), hp))
    model = Tm.Tacotron(inputs=Tm.Tacotron.model_placeholders(), mode=Tm.Mode.PREDICT, engine=eng, hparams=hp)
    ids = bench.synthetic_ids(bench.B_PER_GPU, bench.TS, 1234)
    kw = dict(n_steps=bench.N_STEPS, n_iter=bench.N_ITER, peak_normalize=True)
    logging.getLogger().setLevel(logging.ERROR)   # (peak-normalised rows reach +1 and clip there: not this tool's news)
    logging.basicConfig()
    settings = [('off', None), ('pcm16', 'pcm16'), ('mulaw 8 kHz', ('mulaw', 'tpdf', 8000))]
    for rep in range(args.repeats):
        for name, output in settings:
            for _ in Inf.synthesize_stream(model, (ids for _ in range(max(2, args.warmup))), output=output, **kw):
                pass
            eng.synchronize()
            t0 = time.perf_counter()
            checksum, nbytes = 0.0, 0
            for wavs in Inf.synthesize_stream(model, (ids for _ in range(args.steps)), output=output, **kw):
                checksum += float(wavs[0, 1000])   # the host really reads what came back
                nbytes = wavs.nbytes
            eng.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            assert np.isfinite(checksum)
            print('{:12s} round {}: {:8.3f} ms per step, {:6.2f} MB per answer'.format(name, rep, ms, nbytes / 1e6), flush=True)


stream() if args.stream else stage()
