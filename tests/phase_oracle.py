"""Sequential numpy restatement of the estimated initial phases for Griffin-Lim: the yardstick the
kernels of csrc/phase_init.hip are held to, bit for bit.  Written from the definition, one frame after the other and one bin
after the other; nothing here knows how the kernels cut the work.

Phases are turns in unsigned 32-bit fixed point (angle = 2 pi phi / 2^32, additions wrap), phi_{-1} = 0.  Per frame, on the
float32 magnitudes m:
  * bin j, 1 <= j <= F - 2, is a PEAK if m[j] > m[j-1] and m[j] > m[j+1]; then, in double and in this order,
        p = 0.5 * (a - g) / ((a - 2.0 * b) + g);   x = (hop * (j + p)) / n_fft;   fr = x - floor(x)
        adv = (uint32)floor(fr * 4294967296.0);    phi_t[j] = phi_{t-1}[j] + adv
    (a peak whose fr is not finite -- a neighbour of -Inf -- advances by 0: the conversion is undefined there)
  * a bin k that is no peak walks right while m[i] < m[i+1]; a walk that ends at a peak j is owned by it.  Otherwise it
    walks left while m[i] < m[i-1], likewise.  Ties, edges and NaN end a walk without an owner.
  * an owned bin takes phi_t[j] + ((k - j) & 1) * 2^31, any other keeps phi_{t-1}[k].
The public value is u[k, t] = float32(phi_t[k] >> 8) * 2^-24, exact and in [0, 1).
"""
import math

import numpy as np

TWO32 = 4294967296.0


def peak_advance(a, b, g, j, hop_length, n_fft):
    """adv of a peak at bin j with the float32 neighbours a, b, g -- IEEE double, every operation rounded on its own."""
    a, b, g = np.float64(np.float32(a)), np.float64(np.float32(b)), np.float64(np.float32(g))
    with np.errstate(all='ignore'):
        p = np.float64(0.5) * (a - g) / ((a - np.float64(2.0) * b) + g)
        x = (np.float64(hop_length) * (np.float64(j) + p)) / np.float64(n_fft)
        fr = x - np.floor(x)
    if not np.isfinite(fr):
        return 0
    return int(math.floor(float(fr * np.float64(TWO32)))) & 0xFFFFFFFF


def frame_owners(m):
    """-> (is_peak [F] bool, owner [F] int: the owning peak of a bin that is no peak, -1 for none or for a peak)."""
    m = np.asarray(m, dtype=np.float32)
    F = m.shape[0]
    peak = np.zeros(F, dtype=bool)
    for j in range(1, F - 1):
        peak[j] = bool(m[j] > m[j - 1]) and bool(m[j] > m[j + 1])
    # where the walk from k ends: one step, then where the walk from the neighbour ends (the walks of a ramp share their tail,
    # so each is taken once instead of F times)
    lt = m[:-1] < m[1:]    # lt[i]: m[i] < m[i+1]
    gt = m[1:] < m[:-1]    # gt[i]: m[i+1] < m[i]
    right = list(range(F))
    for i in range(F - 2, -1, -1):
        if lt[i]:
            right[i] = right[i + 1]
    left = list(range(F))
    for i in range(1, F):
        if gt[i - 1]:
            left[i] = left[i - 1]
    owner = np.full(F, -1, dtype=np.int64)
    for k in range(F):
        if peak[k]:
            continue
        if peak[right[k]]:
            owner[k] = right[k]
        elif peak[left[k]]:
            owner[k] = left[k]
    return peak, owner


def phase_track(mag, n_fft, hop_length, n_frames=None):
    """mag (F, T) float32 -> phi (F, T) uint32, frames t >= n_frames left 0 (the kernels do not write them)."""
    mag = np.asarray(mag, dtype=np.float32)
    F, T = mag.shape
    assert F == 1 + n_fft // 2, (F, n_fft)
    n = T if n_frames is None else int(n_frames)
    phi = np.zeros((F, T), dtype=np.uint32)
    prev = np.zeros(F, dtype=np.uint64)
    for t in range(n):
        m = mag[:, t]
        peak, owner = frame_owners(m)
        cur = prev.copy()
        for j in np.flatnonzero(peak):
            cur[j] = (int(prev[j]) + peak_advance(m[j - 1], m[j], m[j + 1], int(j), hop_length, n_fft)) & 0xFFFFFFFF
        for k in np.flatnonzero(owner >= 0):
            j = int(owner[k])
            cur[k] = (int(cur[j]) + (((int(k) - j) & 1) << 31)) & 0xFFFFFFFF
        phi[:, t] = cur.astype(np.uint32)
        prev = cur
    return phi


def phase_to_unit(phi):
    """the public float32 value of a fixed-point phase: (phi >> 8) * 2^-24, exact"""
    return ((np.asarray(phi, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def phase_estimate(mag, n_fft, hop_length, n_frames=None, fill=0.0):
    """mag (F, T) or (B, F, T) float32 -> init_phase of the same shape, float32 in [0, 1): what tts_phase_estimate writes.
    n_frames: a length, or B of them; frames behind an utterance's end hold ``fill`` (the library leaves them untouched)."""
    mag = np.asarray(mag, dtype=np.float32)
    if mag.ndim == 2:
        out = phase_to_unit(phase_track(mag, n_fft, hop_length, n_frames))
        if n_frames is not None:
            out[:, int(n_frames):] = fill
        return out
    B = mag.shape[0]
    lens = [None] * B if n_frames is None else [int(v) for v in np.asarray(n_frames).reshape(-1)]
    assert len(lens) == B
    return np.stack([phase_estimate(mag[b], n_fft, hop_length, lens[b], fill) for b in range(B)])
