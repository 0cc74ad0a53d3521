"""Inputs of the resampler's tests (a plain helper module, imported like stretch_cases.py): the ratios, the ragged batch and the
impulses that tts_resample is held to the oracle on -- test_gpu_resample.py runs them on the device, test_resample_host.py holds
the oracle to its own properties and the bound to its model on the same arrays.  The oracle's results are computed once per case
and shared."""
import numpy as np

import resample_oracle as R

# slower and faster, a table step that is a power of two (0.25, 0.5, >= 1) and one that resampy truncates (2 ** (-4 / 12):
# step 406, 16000 / 22050: step 371), 1.0 (which runs the filter), and the range's ends
RATIOS = [0.25, 0.5, 2.0 ** (-4.0 / 12.0), 16000.0 / 22050.0, 1.0, 2.0 ** (3.0 / 12.0), 2.0, 4.0]
RATIO_IDS = ['0.25', '0.5', 'down4st', '16k-22k', '1.0', 'up3st', '2.0', '4.0']
CLEAN_RATIOS = [0.25, 0.5, 2.0 ** (3.0 / 12.0), 2.0, 4.0]          # exact step: DC and a sine come back to 1e-6
TRUNCATED_RATIOS = [2.0 ** (-4.0 / 12.0), 16000.0 / 22050.0]      # resampy's truncated step: a DC error of 1e-4 .. 1e-3

# one sample, two, a wave less one, a wave, more than one workgroup's tile at every ratio, and several tiles
RAGGED = [1, 2, 63, 64, 700, 5000]
RAGGED_N = 5000
# the same six utterances spread over more than one launch's 64: groups of eight and single utterances, both launches
SPREAD_B = 65
SPREAD_AT = [0, 7, 8, 33, 63, 64]

IMPULSE_N = 700
IMPULSE_AT = [0, 1, IMPULSE_N // 2, IMPULSE_N - 2, IMPULSE_N - 1]

_cache = {}


def ragged_batch():
    """(6, 5000) float32 noise over four decades; NaN at and behind every utterance's length: what a kernel must never read"""
    rng = np.random.default_rng(2026)
    x = (rng.standard_normal((len(RAGGED), RAGGED_N)) * np.power(10.0, rng.integers(-3, 1, (len(RAGGED), RAGGED_N)))).astype(np.float32)
    for b, n in enumerate(RAGGED):
        x[b, n:] = np.nan
    return x


def spread_batch():
    """the ragged batch's utterances at SPREAD_AT of a batch of 65, short noise utterances everywhere else"""
    rng = np.random.default_rng(65)
    x = rng.standard_normal((SPREAD_B, RAGGED_N)).astype(np.float32)
    ns = np.full(SPREAD_B, 40, np.int32)
    ns[1::3] = 300
    rag = ragged_batch()
    for b, at in enumerate(SPREAD_AT):
        x[at] = rag[b]
        ns[at] = RAGGED[b]
    for b in range(SPREAD_B):
        x[b, ns[b]:] = np.nan
    return x, ns


def impulse_batch():
    """(5, 700): a single 1.0 at sample 0, 1, n / 2, n - 2 and n - 1 -- output t is then ONE tap of ONE phase"""
    x = np.zeros((len(IMPULSE_AT), IMPULSE_N), np.float32)
    for b, at in enumerate(IMPULSE_AT):
        x[b, at] = 1.0
    return x


def n_out_choices(longest, rho):
    """N_out below, at and above ceil(longest * rho)"""
    full = R.resampled_length(longest, rho)
    return [max(1, full - 37), full, full + 300]


def oracle(name, rho):
    """(y64, sabs) of a named batch at a ratio, rows of ceil(longest * rho) + 300 samples; computed once"""
    key = (name, rho)
    if key not in _cache:
        if name == 'ragged':
            x, ns = ragged_batch(), RAGGED
        elif name == 'impulse':
            x, ns = impulse_batch(), None
        else:
            raise KeyError(name)
        longest = max(ns) if ns is not None else x.shape[1]
        _cache[key] = R.resample_batch(np.nan_to_num(x.astype(np.float64), nan=0.0) if ns is not None else x, rho, ns,
                                       n_out=R.resampled_length(longest, rho) + 300)
    return _cache[key]


def fit(a, N):
    """rows cut or zero-padded to N samples (fix_length)"""
    out = np.zeros((a.shape[0], N), a.dtype)
    m = min(N, a.shape[1])
    out[:, :m] = a[:, :m]
    return out
