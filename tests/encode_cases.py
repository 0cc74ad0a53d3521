"""The rows the delivery encoder's tests share (tests/test_encode_host.py, tests/test_gpu_encode.py): every 16-bit level, the
special values with what the rules of include/sstts_hip.h make of them, the ties, and seeded speech-like rows."""
import numpy as np

import encode_oracle as O

LSB = 1.0 / 32768.0


def all_levels():
    """x = k / 32768 for k = -32768 .. 32767: float32 holds every one exactly, and pcm16 without dither returns k"""
    return (np.arange(-32768, 32768, dtype=np.float64) / 32768.0).astype(np.float32)


# (a sample, the pcm16 value the rules give it without dither, clipped, nan)
SPECIALS = [
    (1.0, 32767, 1, 0),                        # 32768 is outside: saturated and counted
    (-1.0, -32768, 0, 0),                      # -32768 is inside: not a clip
    (np.float32(1.0) - np.float32(2.0 ** -24), 32767, 1, 0),   # the float below 1: 32767.998 rounds to 32768, outside
    (-0.0, 0, 0, 0),
    (0.0, 0, 0, 0),
    (1e-45, 0, 0, 0),                          # the smallest denormal
    (-1e-40, 0, 0, 0),                         # a denormal
    (np.inf, 32767, 1, 0),
    (-np.inf, -32768, 1, 0),
    (np.nan, 0, 0, 1),
    (3.0e38, 32767, 1, 0),
    (-3.0e38, -32768, 1, 0),
    (0.5 * LSB, 0, 0, 0),                      # ties go to the even integer
    (-0.5 * LSB, 0, 0, 0),
    (1.5 * LSB, 2, 0, 0),
    (-1.5 * LSB, -2, 0, 0),
    (2.5 * LSB, 2, 0, 0),
    (-2.5 * LSB, -2, 0, 0),
    (32766.5 * LSB, 32766, 0, 0),
    (32767.5 * LSB, 32767, 1, 0),              # the tie goes up to 32768: outside
    (-32768.5 * LSB, -32768, 0, 0),            # the tie goes to -32768: inside
    (-32769.5 * LSB, -32768, 1, 0),            # -32770: outside
    (0.25, 8192, 0, 0),
    (-0.75, -24576, 0, 0),
]


def specials():
    """-> (row float32, pcm16 values, clipped, nans, peak): the special values and what they encode to without dither"""
    x = np.array([s[0] for s in SPECIALS], np.float32)
    q = np.array([s[1] for s in SPECIALS], np.int64)
    return x, q, sum(s[2] for s in SPECIALS), sum(s[3] for s in SPECIALS), int(np.abs(q).max())


def speech_like(n, peak=0.9, seed=0):
    """a seeded row of n samples: a few partials under a slow envelope, with a sample over full scale now and then"""
    rng = np.random.default_rng(seed + 1000 * n)
    t = np.arange(n, dtype=np.float64)
    x = sum(rng.uniform(0.1, 0.4) * np.sin(2 * np.pi * f * t / 22050.0 + rng.uniform(0, 6.28)) for f in (110.0, 523.0, 1760.0, 4186.0))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * t / 997.0)) + 0.01 * rng.standard_normal(n)
    x = peak * x / max(np.abs(x).max(), 1e-9)
    if n > 4:
        x[rng.integers(0, n, size=max(1, n // 300))] *= 1.3
    return x.astype(np.float32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_records(got, want):
    return all(np.array_equal(np.asarray(got[name]), np.asarray(want[name])) for name in O.RECORD.names)
