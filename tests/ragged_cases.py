"""Inputs and float64 references of the ragged Griffin-Lim tests (a plain helper module, imported like audio_cases.py).

An utterance's spectrogram and initial phases depend on its configuration and its OWN length alone (the generator is
seeded with them), so the same utterance is the same array in whatever batch, order and padding it appears:
test_ragged_gl_host.py holds a float32 restatement to a quarter of the bounds on exactly what test_gpu_ragged_gl.py feeds
the kernels.  References (oracle.audio_oracle.griffin_lim_v2, tests/momentum_oracle.py) are computed once per utterance
and shared."""
import numpy as np

import audio_cases as C
import momentum_oracle as M
from oracle import audio_oracle as A

STREAM = (2048, 1102, 275)         # (n_fft, win, hop): gl_stream_kernel's first window
STREAM_800 = (2048, 800, 200)      # ... and its second
GENERAL_1024 = (1024, 800, 200)    # the general kernels
GENERAL_512 = (512, 400, 100)

# 5 frames: the shortest legal utterance at 1102 / 275; 8 and 9 straddle "no interior frame" (2 halo + 1 = 9); a long
# utterance followed by a short one
STREAM_LENGTHS = [5, 8, 9, 40, 23]
STREAM_800_LENGTHS = [7, 30, 12]
GENERAL_1024_LENGTHS = [4, 25, 9]
GENERAL_512_LENGTHS = [4, 21, 6]
MOMENTUM_LENGTHS = [5, 9, 40]
MOMENTUM = 0.99

# the table the float32 margin is held on: (config, lengths, iterations)
HOST_TABLE = [(STREAM, [5, 8, 9, 23, 40], 4), (STREAM, [5, 9], 1), (STREAM_800, [7, 12, 30], 4),
              (GENERAL_1024, [4, 9, 25], 3), (GENERAL_512, [4, 6, 21], 3)]


def utterance(cfg, T):
    """(mag (F, T), init (F, T)) of the utterance of T frames: audio_cases.synth_mag at its own length for the streaming
    configurations, power4_mag (what GL_OTHER_SIZES uses) for the general kernels"""
    n_fft, win, hop = cfg
    rng = np.random.default_rng([n_fft, win, hop, T])
    F = 1 + n_fft // 2
    if n_fft == 2048:
        mag = C.synth_mag(rng, 1, T, n_fft, hop, win)[0]
    else:
        mag = C.power4_mag(rng, (F, T))
    return mag, rng.random((F, T)).astype(np.float32)


def batch(cfg, lengths, fill=0.0):
    """the utterances embedded in (B, F, T_max) arrays; `fill` is what the padding columns hold"""
    F, T_max = 1 + cfg[0] // 2, max(lengths)
    mag = np.full((len(lengths), F, T_max), fill, np.float32)
    init = np.full((len(lengths), F, T_max), fill, np.float32)
    for b, T in enumerate(lengths):
        mag[b, :, :T], init[b, :, :T] = utterance(cfg, T)
    return mag, init


_REF = {}


def reference(cfg, T, n_iter, momentum=0.0, init=None, key=None):
    """(waveform, mse) of the float64 oracle for the utterance of T frames; computed once"""
    k = (cfg, T, n_iter, momentum, key)
    if k not in _REF:
        mag, own = utterance(cfg, T)
        u = own if init is None else init
        n_fft, win, hop = cfg
        if momentum:
            _REF[k] = M.griffin_lim_momentum(mag, win, hop, n_fft, n_iter, u, momentum=momentum)
        else:
            _REF[k] = A.griffin_lim_v2(mag, win, hop, n_fft, n_iter, init_phase=u)
    return _REF[k]
