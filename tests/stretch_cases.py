"""Inputs of the speaking-rate tests (a plain helper module, imported like eos_cases.py): the small batches that the stretch
kernels are held to the oracle on -- test_gpu_stretch.py runs them on the device, test_stretch_host.py holds the oracle's
round-once blend to its whole phase-vocoder path on the same arrays."""
import numpy as np

import stretch_oracle as S

# every rate class: slower (0.5, 0.75), off (1.0), faster with and without a fractional step (1.3, 2.0, 3.7)
STAGE_RATES = [0.5, 0.75, 1.0, 1.3, 2.0, 3.7]
STAGE_B, STAGE_T = 3, 12
STAGE_F = [1025, 129, 1]        # rows of 1025 floats start at every alignment; one 16-byte load and one float; one bin
STAGE_LENGTHS = [12, 7, 1]      # full, odd, the shortest
PAD = 3                         # time-major rows: F + 3 floats (a multiple of 4 for every F above: the 16-byte path)

# the rates of the frame-count and full-path checks (the issue's list)
HOST_RATES = [0.5, 0.75, 0.8, 1.25, 1.3, 2.0, 3.7]
HOST_T = [1, 7, 12, 25, 40]


def stage_batch(F, B=STAGE_B, T=STAGE_T):
    """(B, F, T) float32 magnitudes in the reference layout: positive, spread over six decades, with exact zeros (a whole
    column and single bins) so that 'zero stays zero' is exercised"""
    rng = np.random.default_rng([F, T, B])
    x = (rng.random((B, F, T)) * np.power(10.0, rng.integers(-4, 2, (B, F, T)))).astype(np.float32)
    x[:, :, T // 2] = 0.0
    x[0, F // 2, 1] = 0.0
    return x


def stage_phases(F, B=STAGE_B, T=STAGE_T):
    return np.random.default_rng([F, T, B, 1]).uniform(-np.pi, np.pi, (B, F, T))


def poisoned(x, n_frames):
    """x with NaN in every column at or behind n_frames[b]: what a kernel must never read"""
    y = x.copy()
    if n_frames is not None:
        for b, n in enumerate(n_frames):
            y[b, :, n:] = np.nan
    return y


def time_major(x_ft, pad=PAD, fill=np.nan):
    """(B, F, T) -> the contiguous (B, T, F + pad) array that holds it time-major, padding columns = fill"""
    B, F, T = x_ft.shape
    full = np.full((B, T, F + pad), fill, np.float32)
    full[:, :, :F] = x_ft.transpose(0, 2, 1)
    return full


def longest(n_frames, T, rate):
    return max(S.stretched_frames(n, rate) for n in (n_frames if n_frames is not None else [T]))
