"""The cases of the F0 tests, shared by the host tests (tests/test_f0_host.py) and the GPU tests (tests/test_gpu_f0*.py): the
parameter grid, the lengths placed round a hop and a span, the waveform contents, the tones of known pitch and the F0 tracks of
the comparison."""
import numpy as np

SR = 22050
# (W, tau_min, tau_max, hop): the smallest call, one lag short of a wave / a wave / one beyond it, the evaluation's, the limits
GRID = [(1, 2, 2, 1), (63, 2, 63, 7), (64, 2, 64, 64), (65, 3, 65, 300), (1024, 44, 368, 275), (2048, 2, 1024, 512)]
THRESHOLDS = [0.1, 0.0, float('inf')]     # the default, never voiced, always voiced
CONTENTS = ['zeros', 'constant', 'integers', 'tone', 'subharmonic', 'noise', 'fading', 'tiny', 'huge', 'nan', 'inf']
TONES_HZ = [70.0, 110.0, 150.0, 220.0, 333.0, 450.0]
EVAL = dict(hop=275, W=1024, tau_min=44, tau_max=368)     # sr 22050, 60 .. 500 Hz


def lengths(W, tau_max, hop):
    span = W + tau_max
    return sorted({n for n in (1, hop - 1, hop, hop + 1, span - 1, span + 1, 3 * span + 5) if n >= 1})


def tone(hz, n, sr=SR, partials=7, seed=0, amplitude=0.5):
    """a harmonic tone: `partials` partials of amplitude 1 / k with random phases"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros(n, np.float64)
    for k in range(1, partials + 1):
        x += np.sin(2.0 * np.pi * hz * k * t + rng.uniform(0, 2.0 * np.pi)) / k
    return (amplitude * x / np.abs(x).max()).astype(np.float32) if n else x.astype(np.float32)


def content(kind, n, tau_max, seed=0):
    """(n,) float32; the period of the tones is placed inside the lags searched"""
    rng = np.random.default_rng([seed, n, tau_max, CONTENTS.index(kind)])
    period = max(2.0, 0.37 * tau_max + 1.3)
    k = np.arange(n, dtype=np.float64)
    wave = np.sin(2.0 * np.pi * k / period) + 0.4 * np.sin(4.0 * np.pi * k / period + 1.0)
    if kind == 'zeros':
        x = np.zeros(n)
    elif kind == 'constant':
        x = np.full(n, 0.75)
    elif kind == 'integers':
        x = rng.integers(-8, 9, n).astype(np.float64)
    elif kind == 'tone':
        x = 0.5 * wave
    elif kind == 'subharmonic':
        x = 0.5 * wave + 0.45 * np.sin(np.pi * k / period + 0.3)
    elif kind == 'noise':
        x = rng.standard_normal(n)
    elif kind == 'fading':
        x = 0.5 * wave * np.clip(1.0 - 1.5 * k / max(n, 1), 0.0, 1.0)
    elif kind == 'tiny':
        x = 1e-30 * wave
    elif kind == 'huge':
        x = 1e30 * (wave + 0.1 * rng.standard_normal(n))
    elif kind in ('nan', 'inf'):
        x = 0.5 * wave + 0.01 * rng.standard_normal(n)
        x[(2 * n) // 3] = np.nan if kind == 'nan' else np.inf
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def batch(n, tau_max, seed=0):
    """(len(CONTENTS), n) float32: every content at one length"""
    return np.stack([content(kind, n, tau_max, seed) for kind in CONTENTS])


def tracks(seed, Ta, Tb):
    """two F0 tracks in Hz for the comparison: voiced and unvoiced stretches, NaNs, equal values, a pair exactly at the 20 % edge
    and values one float apart -- placed along the diagonal, where a path between similar tracks runs"""
    rng = np.random.default_rng(seed)
    a = (120.0 + 40.0 * rng.random(Ta)).astype(np.float32)
    b = (120.0 + 40.0 * rng.random(Tb)).astype(np.float32)
    m = min(Ta, Tb)
    if m >= 20:
        a[2:5] = 0.0                         # one side unvoiced
        b[7:9] = 0.0
        a[11:13], b[11:13] = 0.0, 0.0        # both unvoiced
        a[14] = np.nan
        b[16] = np.nan
        a[17], b[17] = np.float32(180.0), np.float32(150.0)        # |u| = 30 = 0.2 * 150 exactly in double: no gross error
        a[18], b[18] = np.nextafter(np.float32(180.0), np.float32(1e9)), np.float32(150.0)   # one float beyond the edge
        a[19] = b[19] = np.float32(133.25)                          # equal
    if m >= 24:
        a[20], b[20] = np.float32(200.0), np.nextafter(np.float32(200.0), np.float32(0.0))   # one float apart
        a[21], b[21] = np.float32(100.0), np.float32(400.0)         # two octaves
        a[22], b[22] = np.float32(-0.0), np.float32(140.0)          # -0.0 is unvoiced
    return a, b


def diagonal_path(na, nb, rows):
    """a legal path from (0, 0) to (na - 1, nb - 1) in `rows` rows, (-1, -1) behind it"""
    path = np.full((rows, 2), -1, np.int32)
    i = j = k = 0
    path[0] = (0, 0)
    while (i, j) != (na - 1, nb - 1):
        if i < na - 1 and j < nb - 1:
            i, j = i + 1, j + 1
        elif i < na - 1:
            i += 1
        else:
            j += 1
        k += 1
        path[k] = (i, j)
    return path
