"""Inputs and parameter sets of the watermark tests: speech-like signals made here -- harmonic tones under a syllable-rate amplitude
modulation with pauses of exact zeros -- each seeded by its own length so that it is the same in every batch it appears in.
Nothing is read from anywhere.  No GPU, no library."""
import numpy as np

import watermark_oracle as O
from equalizer_cases import FILL, bits, padded, same   # noqa: F401

SR = 22050
KEY = 0x5EEDC0DE12345678
# (payload, payload_bits, chip, chips_per_symbol, strength): L = 2, 8, 16; C = 1 and 16; P = 1, 8, 32
SETS = {
    'default': (0xA5C3, 16, 8, 64, 0.02),
    'narrow': (0x1, 1, 2, 1, 0.05),
    'byte': (0x9D, 8, 8, 16, 0.03),
    'wide': (0xDEADBEEF, 32, 16, 1, 0.04),
    'odd_chip': (0x2B, 6, 6, 5, 0.02),
    'short': (0x35, 8, 2, 16, 0.05),           # a symbol of 32 samples: its border lies inside 64 offsets
}


def params(name, key=KEY, **over):
    payload, P, L, C, G = SETS[name]
    return O.params(key, payload, P, L, C, G)._replace(**over)


def voiced(n, f0=140.0, amp=0.5, seed=None, sr=SR):
    """harmonics of ``f0`` with a slow vibrato under a syllable-rate modulation; every third syllable or so is a pause of zeros"""
    rng = np.random.RandomState(n if seed is None else seed)
    t = np.arange(n) / float(sr)
    phase = 2 * np.pi * f0 * t + 0.8 * np.sin(2 * np.pi * 5.1 * t + rng.rand())
    x = np.zeros(n)
    for h in range(1, 16):
        x += np.sin(h * phase + 2 * np.pi * rng.rand()) / h ** 0.9
    x += 0.05 * rng.randn(n)                                   # breath
    syll = int(0.18 * sr)
    env = np.abs(np.sin(np.pi * np.arange(n) / syll)) ** 0.7
    pause = (rng.rand(n // syll + 1) < 0.3)[np.arange(n) // syll]
    env[pause] = 0.0
    x *= env
    return (amp * x / max(1e-9, np.abs(x).max(initial=0.0))).astype(np.float32)


def signals(n=20000):
    """the signals the threshold is measured on"""
    return {'low': voiced(n, 110.0, seed=1), 'mid': voiced(n, 170.0, seed=2), 'high': voiced(n, 240.0, amp=0.8, seed=3),
            'quiet': voiced(n, 140.0, amp=0.02, seed=4)}


def specials(n):
    """NaN, +-Inf, -0.0 and float32 denormals among voiced samples"""
    x = voiced(n, seed=n + 3)
    tiny = np.float32(1e-45)
    for i, v in ((0, np.nan), (1, -0.0), (2, tiny), (70, np.inf), (n // 3, np.float32(1.1e-39)), (n // 3 + 1, -0.0),
                 (2 * n // 3, -np.inf), (2 * n // 3 + 2, np.nan), (n - 1, -0.0)):
        if 0 <= i < n:
            x[i] = v
    return x


def denormal(n):
    rng = np.random.RandomState(n + 11)
    return (rng.randint(-40, 41, n) * np.float32(1e-45)).astype(np.float32)


def as_engine(p):
    """the oracle's parameters as ``Engine.watermark_embed`` and ``watermark_detect`` take them"""
    return tuple(p)


# ---- the robustness chain (tests/test_gpu_watermark_chain.py on the device, tests/test_watermark_host.py on the oracles alone):
# embed, limiter, resample to 8000 Hz, mu-law, decode by table, resample back, detect.  The strength and the length are chosen so
# that the oracles alone pass with zeta at least twice the threshold (the host test records the margin).
CHAIN_SR, CHAIN_RATE = SR, 8000
CHAIN_N, CHAIN_CUT, CHAIN_OFFSETS = 20000, 37, 64
CHAIN_CEILING, CHAIN_LOOKAHEAD = 0.5, 110
CHAIN_WRONG_KEY = 77


def chain_params():
    return params('default', strength=0.2)


def chain_signal():
    return voiced(CHAIN_N, 170.0, amp=0.6, seed=2)


def chain_on_the_oracles(x, p, cut=CHAIN_CUT):
    """the received row at CHAIN_SR after the chain, on the numpy oracles of every stage"""
    import encode_oracle as EO
    import limiter_oracle as LO
    import resample_oracle as RO
    y = O.embed(x, p)[0][cut:]
    y = LO.limit(y, LO.design(), CHAIN_CEILING, CHAIN_LOOKAHEAD, 4)[0]
    down = RO.resample(y, float(CHAIN_RATE) / CHAIN_SR)[0].astype(np.float32)
    codes = EO.encode_row(down, EO.MULAW)[0]
    return RO.resample(mulaw_decode(codes), float(CHAIN_SR) / CHAIN_RATE)[0].astype(np.float32)


def mulaw_decode(codes):
    """G.711 mu-law codes to float32 by table"""
    import encode_oracle as EO
    return (EO.decode(EO.MULAW, np.asarray(codes, np.uint8)).astype(np.float32) * np.float32(1.0 / 32768.0)).astype(np.float32)
