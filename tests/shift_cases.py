"""Inputs of the formant-preserving pitch tests (a plain helper module): the frames, the segment lists and how the library is
called with a guard band around its output.  A segment is a row ``(row, first, frames, pitch_step, formant_step)``.  The shapes
are the smallest at which the kernel can still go wrong: T = 70 (tiles of 8 frames: segments of 7, 8 and 9 frames, a rest of the
row longer than one copy tile of 64), B of 1 .. 3, F = 1025 and once each 129 and 2049."""
import ctypes

import numpy as np

import segment_cases as SC
import shift_oracle as O
from segment_cases import NAN_PATTERN, poisoned   # noqa: F401 (re-exported)

TILE = O.TILE
PER_LAUNCH = O.SEGMENTS_PER_LAUNCH
SR, N_FFT, WIN = 22050, 2048, 1102  # the listening test's analysis
TONES = (100.0, 150.0, 220.0)
UP4, DOWN4 = O.step(4), O.step(-4)


def tone_amplitude(f):
    """the two-formant envelope of the listening test"""
    f = np.asarray(f, dtype=np.float64)
    return 1.0 / (1.0 + ((f - 700.0) / 300.0) ** 2) + 0.5 / (1.0 + ((f - 2200.0) / 400.0) ** 2) + 0.02


def tone(f0, n, seed, sr=SR):
    """n samples of a harmonic tone of f0 Hz: every harmonic up to Nyquist under ``tone_amplitude``, with seeded random phases"""
    rng = np.random.default_rng([int(round(f0)), seed])
    h = np.arange(1, int((sr / 2) // f0) + 1, dtype=np.float64) * f0
    h = h[h < sr / 2]
    ph = rng.random(h.shape[0]) * 2 * np.pi
    t = np.arange(n, dtype=np.float64) / sr
    return (tone_amplitude(h)[:, None] * np.cos(2 * np.pi * h[:, None] * t[None, :] + ph[:, None])).sum(axis=0)


def tone_frame(f0, seed=0):
    """one magnitude frame (1025,) float32 of the tone: a Hann window of 1102 samples in an n_fft of 2048"""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(WIN) / WIN)
    return np.abs(np.fft.rfft(tone(f0, WIN, seed) * w, N_FFT)).astype(np.float32)


def harmonic_case():
    """(1, 1025, 3): the three tones' frames, the case the float32 and the lifter variants are judged on"""
    return np.stack([tone_frame(f) for f in TONES], axis=1)[None]


def batch(B, F, T):
    """(B, F, T) float32 magnitudes: harmonics of 80 .. 300 Hz (bin widths scaled to F) under a two-formant envelope on a noise
    floor, the frames spread over four decades of level"""
    rng = np.random.default_rng([F, T, B, 23])
    f = np.arange(F, dtype=np.float64) * (SR / 2) / (F - 1)
    f0 = rng.uniform(80.0, 300.0, (B, 1, T))
    d = (f[None, :, None] / f0 + 0.5) % 1.0 - 0.5                      # distance to the nearest harmonic, in harmonics
    comb = np.exp(-(d * f0 / 25.0) ** 2)
    level = np.power(10.0, rng.uniform(-3, 1, (B, 1, T)))
    x = level * (tone_amplitude(f)[None, :, None] * comb + 1e-3 * rng.random((B, F, T)))
    return x.astype(np.float32)


def with_specials(x):
    """x (rows of at least 40 frames) with, in row 0: a NaN in frame 4 and an Inf in frame 10 (computed frames of ``mixed``), an
    all-zero frame 22, denormal bins in frame 36, a negative bin in frame 37, a frame of denormals alone (38); and in the copied
    frames 30 and 31 a NaN with a payload and a -0.0"""
    x = x.copy()
    F = x.shape[1]
    x[0, min(100, F - 1), 4] = np.nan
    x[0, 0, 10] = np.inf
    x[0, :, 22] = 0.0
    x[0, 3:9, 36] = (1e-42, 3e-45, 1e-39, 1e-42, 1e-40, 2e-41)
    x[0, 5, 37] = -x[0, 5, 37]
    x[0, :, 38] = (x[0, :, 38].astype(np.float64) * 1e-40 / max(float(x[0, :, 38].max()), 1e-30)).astype(np.float32)
    x.view(np.uint32)[0, 7, 30] = 0x7fc12345
    x[0, 8, 31] = -0.0
    return x


def mixed():
    """B = 3, T = 70, ragged: uncovered gaps in front, between and behind; segments of TILE - 1, TILE and TILE + 1 frames; the pitch
    step alone, the formant step alone, both; folding (pitch_step > 65536); both ends of the range; a copy segment; a whole row; a
    row with one computed frame"""
    n = [70, 41, 9]
    seg = [(0, 2, TILE - 1, UP4, O.UNITY),              # the pitch alone; frames 0, 1 in front are copies
           (0, 9, TILE, O.UNITY, O.step(-3)),           # the formants alone, adjacent to its predecessor
           (0, 20, TILE + 1, DOWN4, O.step(2)),         # folding, both steps; frames 17 .. 19 are a gap
           (0, 29, 5, O.UNITY, O.UNITY),                # a copy segment
           (0, 34, 17, O.STEP_MIN, O.STEP_MAX),         # the ends of the range, three tiles
           (0, 51, 3, O.STEP_MAX, O.STEP_MIN),
           (0, 60, 10, O.step(7), O.UNITY),             # up to the row's last frame
           (1, 0, 41, UP4, O.UNITY),                    # a whole row of 41 frames: the rest of its T is +0.0
           (2, 3, 1, O.step(-2), O.step(-2))]           # one frame; 0 .. 2 and 4 .. 8 are copies
    return dict(B=3, T=70, n_frames=n, segments=seg)


def launch_seam():
    """B = 2, T = 70: PER_LAUNCH - 4 one-frame segments in row 0 and five in row 1 -- 65 segments, and row 1 straddles two launches"""
    steps = (UP4, O.UNITY, DOWN4, O.step(1), O.STEP_MIN, O.STEP_MAX)
    seg = [(0, s, 1, steps[s % 6], steps[(s // 6) % 6]) for s in range(PER_LAUNCH - 4)]
    seg += [(1, 2 + 12 * j, 1 + 2 * j, steps[j], steps[(j + 2) % 6]) for j in range(5)]
    return dict(B=2, T=70, n_frames=[70, 66], segments=seg)


LISTS = dict(mixed=mixed, launch_seam=launch_seam)


def segment_array(H, segments):
    """the rows as the contiguous SHIFT_SEGMENT array the library reads (unchecked: refusals travel through it too); six fields:
    ``reserved`` in fourth place"""
    return SC.segment_array(H.SHIFT_SEGMENT, segments)


def raw_shift(eng, H, x, n_frames, segments, order, shift=0, S=None, B=None, F=None, T=None, in_place=False):
    """tts_shift_magnitudes through the library itself: ``x`` (B, F, T) host floats go into a buffer ``shift`` floats behind an
    allocation's start, the result into one that holds NAN_PATTERN everywhere and starts ``shift`` floats behind its own:
    ``(return code, out (B, F, T) as uint32 bits, the words around it)``"""
    Bx, Fx, Tx = x.shape
    q = segment_array(H, segments)
    total = Bx * Fx * Tx
    src = eng.to_device(np.concatenate([np.full(shift, np.nan, np.float32), x.ravel()]))
    buf = eng.to_device(np.full(total + 16, NAN_PATTERN, np.uint32))
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
    try:
        p_in = src.data_ptr() + 4 * shift
        rc = eng.lib.tts_shift_magnitudes(eng.handle, p_in, Bx if B is None else B, Fx if F is None else F, Tx if T is None else T,
                                          None if nf is None else nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), q.ctypes.data,
                                          len(q) if S is None else S, int(order), p_in if in_place else buf.data_ptr() + 4 * (8 + shift))
        host = buf.to_host()
    finally:
        buf.free()
        src.free()
    lo = 8 + shift
    return rc, host[lo:lo + total].reshape(Bx, Fx, Tx), np.concatenate([host[:lo], host[lo + total:]])
