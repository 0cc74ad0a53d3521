#!/usr/bin/env python3
"""Dataset feature pass benchmark (csrc/features.hip): seeded LJ-like recordings (1-10 s at 22.05 kHz, voiced tones with a
syllable envelope, a noise floor and silent margins), model configuration (n_fft 2048, 1102 / 275, r = 5, trim top_db 60).

Reports, for batches of --B recordings:
  * extract: plan + extract (device-resident wav, outputs left on the device): audio-seconds / s, recordings / s, device ms of
    the "features" stage (profile events), launches per batch;
  * end to end: 16-bit PCM wav files -> load_wav -> compute_features -> np.savez (DatasetHelper.pre_compute_features);
  * algorithmic bytes (wav read by trim and by the frames, both rows written) and FLOPs (5 N log2 N per complex FFT of
    n_fft / 2 points plus the split pass, the mel products) against the MI355X peaks (8 TB/s HBM, 157 TFLOP/s f32 vector);
  * the float64 numpy pipeline's CPU rate (tests/trim_oracle.py) on a few recordings.

    python tools/feature_bench.py [--B 48] [--batches 4] [--iters 5] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sstts = importlib.import_module('single-speaker-tts_amd')
LJ = importlib.import_module('single-speaker-tts_amd.datasets.lj_speech').LJSpeechDatasetHelper
load_wav = importlib.import_module('single-speaker-tts_amd.audio.io').load_wav
SR = 22050
HBM_PEAK = 8.0e12
VALU_PEAK = 157.3e12


def recording(rng):
    n = int(rng.uniform(1.0, 10.0) * SR)
    t = np.arange(n) / SR
    f0 = rng.uniform(90, 220)
    x = sum(rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.3)) for h in range(1, 12))
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2, 5) * t)
    x = 0.5 * x / np.max(np.abs(x)) + 5e-4 * rng.standard_normal(n)
    lead, trail = int(rng.uniform(0.05, 0.5) * SR), int(rng.uniform(0.05, 0.5) * SR)
    return np.concatenate([1e-4 * rng.standard_normal(lead), x, 1e-4 * rng.standard_normal(trail)]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=48)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--oracle', type=int, default=3, help='recordings timed through the float64 numpy pipeline')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    batches = [[recording(rng) for _ in range(a.B)] for _ in range(a.batches)]
    eng = sstts.Engine()
    p = LJ.feature_params(eng)
    lib, h = eng.lib, eng.handle

    # ---- extract alone: device-resident wav, plan (one sync) + extract, outputs on the device
    staged = []
    for wavs in batches:
        flat, offsets = eng._ragged(wavs)
        staged.append((eng.to_device(flat), offsets, len(wavs)))
    plan = np.zeros(3 * a.B, np.int64)
    outs = {}

    def run(d, offsets, B):
        eng._check(lib.tts_plan_features(h, d.ptr, offsets.ctypes.data, B, eng_p, plan.ctypes.data))
        rows = int(plan[2::3][:B].sum())
        if rows > outs.get('rows', 0):
            for k in ('mel', 'lin'):
                if k in outs:
                    outs[k].free()
            outs['mel'], outs['lin'], outs['rows'] = eng.empty((rows, 80)), eng.empty((rows, 1025)), rows
        eng._check(lib.tts_extract_features(h, d.ptr, offsets.ctypes.data, B, eng_p, plan.ctypes.data, outs['mel'].ptr,
                                            outs['lin'].ptr))
        return rows

    eng_p = __import__('ctypes').byref(p)
    for s in staged:                       # warm-up: tables, workspaces, code objects
        run(*s)
    eng.synchronize()
    eng.set_option('profile', 1)
    eng.profile_reset()
    rows_total = 0
    t0 = time.perf_counter()
    for _ in range(a.iters):
        for s in staged:
            rows_total += run(*s)
    eng.synchronize()
    wall = time.perf_counter() - t0
    dev_ms, launches = eng.profile_get('features')
    eng.set_option('profile', 0)
    n_batches = a.iters * len(staged)
    samples = sum(len(w) for wavs in batches for w in wavs) * a.iters
    audio_s = samples / SR
    recs = a.B * n_batches
    # algorithmic traffic: trim reads every sample once (frames overlap 4x: from cache), frames read ~ win / hop x the
    # samples (from cache) -- counted once; rows written: (80 + 1025) floats per frame
    bytes_alg = samples * 4 * 2 + rows_total * (80 + 1025) * 4
    m = 1024
    flops = rows_total * (5 * m * np.log2(m) + 1024 * 10 + 1025 * 3 + 2 * 1025) + samples * 2 * 4
    r_extract = dict(audio_s_per_s=audio_s / wall, recordings_per_s=recs / wall, device_ms_per_batch=dev_ms / n_batches,
                     wall_ms_per_batch=1e3 * wall / n_batches, launches_per_batch=launches / n_batches,
                     hbm_fraction_of_peak=bytes_alg / (dev_ms * 1e-3) / HBM_PEAK,
                     flop_fraction_of_peak=flops / (dev_ms * 1e-3) / VALU_PEAK)

    # ---- end to end: wav files -> npz
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i, w in enumerate(batches[0]):
            path = os.path.join(tmp, 'r%03d.wav' % i)
            with wave.open(path, 'wb') as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(SR)
                f.writeframes(np.clip(np.round(w * 32767), -32768, 32767).astype('<i2').tobytes())
            paths.append(path)
        helper = LJ(tmp, {'pad': 0, 'eos': 1}, True)
        with contextlib.redirect_stdout(io.StringIO()):
            helper.pre_compute_features(paths, batch_size=a.B, engine=eng)      # warm-up
            t0 = time.perf_counter()
            for _ in range(a.iters):
                helper.pre_compute_features(paths, batch_size=a.B, engine=eng)
            e2e = time.perf_counter() - t0
        a0 = sum(len(w) for w in batches[0]) / SR * a.iters
        t0 = time.perf_counter()
        for _ in range(a.iters):
            for pth in paths:
                load_wav(pth)
        t_load = time.perf_counter() - t0
        r_e2e = dict(audio_s_per_s=a0 / e2e, recordings_per_s=a.B * a.iters / e2e, ms_per_batch=1e3 * e2e / a.iters,
                     load_wav_ms_per_batch=1e3 * t_load / a.iters)

    # ---- numpy float64 oracle on the CPU
    import trim_oracle as T
    ws = batches[0][:a.oracle]
    t0 = time.perf_counter()
    for w in ws:
        T.features(w)
    t_or = time.perf_counter() - t0
    r_or = dict(audio_s_per_s=sum(len(w) for w in ws) / SR / t_or, recordings_per_s=len(ws) / t_or)

    res = dict(tool='feature_bench', B=a.B, batches=a.batches, iters=a.iters, extract=r_extract, end_to_end=r_e2e,
               oracle_cpu=r_or)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    for s in staged:
        s[0].free()
    eng.close()


if __name__ == '__main__':
    main()
