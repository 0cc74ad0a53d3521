"""Inputs of the end-of-speech tests (a plain helper module, imported like ragged_cases.py): the hand-made batches that
tts_speech_frames is held to the oracle on, and the small end-to-end cases -- ids, weights, the choice of a threshold --
that test_gpu_eos.py runs on the device and test_eos_host.py checks on the float64 network oracle.

The end-to-end condition (a condition on the INPUT, not a tolerance): the threshold lies in a gap between the frames'
maxima, at least OFF_THRESHOLD normalised units from every one of them.  The float32 clip / de-normalise / pow of the device
move a value by ~1e-6 relative, so no frame can change sides and the lengths must equal the oracle's exactly."""
import numpy as np

import eos_oracle as E
from conftest import pkg
from oracle import audio_oracle as A

REF_DB, MAX_DB, POWER = 6.02, 99.89, 1.3
RANGE_DB = abs(REF_DB) + abs(MAX_DB)
OFF_THRESHOLD = 1e-3

# ---------------------------------------------------------------------------------------------- tts_speech_frames
STAGE_B, STAGE_T = 5, 37
STAGE_THRESHOLD = np.float32(0.5)
STAGE_F = [1025, 129, 1]


def stage_batch(F, B=STAGE_B, T=STAGE_T, thr=STAGE_THRESHOLD):
    """(B, T, F) float32: a background below the threshold and, by utterance,
    0: a maximum in column 0 (t = 3) and one in column F - 1 (t = 12), then only frames that must NOT count -- a row whose
       maximum EQUALS the threshold (t = 20), a row with a NaN that also holds a value above the threshold (t = 30; with
       F = 1 the NaN alone), a row of -Inf (t = 33): last active frame 12
    1: no active frame;  2: active only at t = 0;  3: active only at t = T - 1
    4: several active frames, the last one (t = 25) through a +Inf"""
    assert B == 5 and T >= 34
    rng = np.random.default_rng([F, T])
    x = (rng.random((B, T, F)) * 0.4).astype(np.float32)
    x[0, 3, 0] = 0.9
    x[0, 12, F - 1] = 0.9
    x[0, 20, F // 2] = thr
    x[0, 30, 0] = np.nan
    if F > 1:
        x[0, 30, F - 1] = 0.9
    x[0, 33, :] = -np.inf
    x[2, 0, F // 3] = 0.7
    x[3, T - 1, (2 * F) // 3] = np.nextafter(thr, np.float32(1))   # the smallest value above the threshold
    x[4, 5, F // 2] = 0.6
    x[4, 17, 0] = 0.8
    x[4, 25, F - 1] = np.inf
    return x


STAGE_EXPECT_LAST = [12, -1, 0, STAGE_T - 1, 25]


def padded(x, pad, fill):
    """x (B, T, F) inside a contiguous (B, T, F + pad) array whose padding columns hold `fill`; returns (the whole array,
    its view [:, :, :F])"""
    B, T, F = x.shape
    full = np.full((B, T, F + pad), fill, np.float32)
    full[:, :, :F] = x
    return full, full[:, :, :F]


# ---------------------------------------------------------------------------------------------- end to end
# the reference architecture (streaming kernel, 1102 / 275: the shortest legal utterance has 5 frames) and one at n_fft = 512
# (general kernels, 400 / 100: 4 frames)
E2E = dict(n_fft=2048, B=3, Ts=12, S=8, n_iter=3, win=1102, hop=275, min_frames=5, ids_seed=2)
E2E_512 = dict(n_fft=512, B=3, Ts=12, S=5, n_iter=3, win=400, hop=100, min_frames=4, ids_seed=2)
# glorot-scale synthetic weights make three utterances that differ by 1e-3 of the scale: no threshold can separate their
# lengths AND stay off every frame's maximum.  An embedding 64 times larger spreads them (still seeded, still synthetic).
EMBEDDING_SCALE = 64.0


def hparams_of(case):
    hp = pkg('tacotron.params').ModelParams()
    hp.n_fft = case['n_fft']
    return hp


_WEIGHTS = {}


def weights_of(case):
    k = case['n_fft']
    if k not in _WEIGHTS:
        w = pkg('tacotron.weights').synthetic_weights(0, hparams_of(case))
        w['encoder/embedding'] = np.ascontiguousarray(w['encoder/embedding'] * np.float32(EMBEDDING_SCALE))
        _WEIGHTS[k] = w
    return _WEIGHTS[k]


def ids_of(case, seed=None):
    """three different kinds of sentence: random characters, one character repeated, a short one followed by padding"""
    rng = np.random.default_rng(case['ids_seed'] if seed is None else seed)
    ids = rng.integers(2, 39, (case['B'], case['Ts'])).astype(np.int32)
    ids[:, -1] = 1
    ids[1, :] = ids[1, 0]
    ids[2, 4:] = 0
    return ids


def init_of(case):
    T = case['S'] * hparams_of(case).reduction
    return np.random.default_rng(11).random((case['B'], 1 + case['n_fft'] // 2, T)).astype(np.float32)


def frames_db(linear_b):
    """one utterance's normalised linear spectrogram (T, F) as the (F, T) float64 dB array the reference's inference() makes of
    it (tacotron/inference.py:96-98, inv_normalize_decibel with the mel constants)"""
    return A.inv_normalize_decibel(np.asarray(linear_b, dtype=np.float64).T, REF_DB, MAX_DB)


def normalised(threshold_db):
    return (float(threshold_db) - REF_DB) / RANGE_DB + 1.0


def distance_from_threshold(linear, threshold_db):
    """the smallest |frame maximum - threshold| over the batch, in normalised units (the data's own, after the clip)"""
    mx = np.clip(np.asarray(linear, dtype=np.float64), 0.0, 1.0).max(axis=2)
    return float(np.abs(mx - normalised(threshold_db)).min())


def oracle_lengths(linear, threshold_db, keep_frames, min_frames):
    out = [E.speech_frames(frames_db(u), float(threshold_db), keep_frames, min_frames) for u in linear]
    return np.array([o[0] for o in out], np.int32)


def choose_threshold(linear, min_frames, keep_frames=0):
    """threshold_db (a float32 value) in the middle of the widest gap between the frames' maxima for which the B lengths all
    differ; None when no gap of at least 2 OFF_THRESHOLD normalised units does that"""
    B = len(linear)
    mx_db = np.stack([E.frame_maxima(frames_db(u)) for u in linear])
    v = np.unique(mx_db.reshape(-1))
    best = None
    for lo, hi in zip(v[:-1], v[1:]):
        if (hi - lo) / RANGE_DB < 2.2 * OFF_THRESHOLD:
            continue
        thr = np.float32((lo + hi) / 2)
        n = oracle_lengths(linear, thr, keep_frames, min_frames)
        if len(set(n.tolist())) == B and (best is None or hi - lo > best[0]):
            best = (hi - lo, thr)
    return None if best is None else best[1]
