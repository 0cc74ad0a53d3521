"""End-of-speech oracle (a plain helper module, imported like trim_oracle.py): a numpy restatement of the reference's
``silence_interval_from_spectrogram`` (audio/effects.py:218-233) -- the criterion its own TODO asks for at
tacotron/inference.py:76-78 and never calls -- plus the clamp that turns the interval's end into a frame count.

Everything is float64 on (F, T) arrays, the reference's layout and ``ref=np.max``.  float32 inputs convert exactly, so a
comparison made here is the comparison tts_speech_frames makes on the float32 data: the results must agree as integers."""
import numpy as np


def frame_maxima(spec_ft):
    """np.max over the bins of every frame (effects.py:219, ref=np.max, axis 0): a NaN anywhere in a frame makes its
    maximum NaN, as numpy propagates it."""
    with np.errstate(invalid='ignore'):
        return np.max(np.asarray(spec_ft, dtype=np.float64), axis=0)


def silence_interval(spec_ft, threshold):
    """effects.py:218-233 on one (F, T) array: (trim_start, trim_end) of the frames whose maximum is strictly above the
    threshold, or None when there is none (a NaN maximum compares False: such a frame is silent)."""
    with np.errstate(invalid='ignore'):
        non_silent = frame_maxima(spec_ft) > np.float64(threshold)     # :221
    nonzero = np.flatnonzero(non_silent.astype(np.int32))              # :222-224
    if len(nonzero) == 0:                                              # :226-227
        return None
    return int(np.min(nonzero)), int(np.max(nonzero))                  # :229-232


def speech_frames(spec_ft, threshold, keep_frames=0, min_frames=1):
    """(n_frames, last_active) of one (F, T) array: last_active = trim_end or -1, n_frames = min(T, max(min_frames,
    last_active + 1 + keep_frames))."""
    T = np.asarray(spec_ft).shape[1]
    interval = silence_interval(spec_ft, threshold)
    last = -1 if interval is None else interval[1]
    return min(T, max(int(min_frames), last + 1 + int(keep_frames))), last


def speech_frames_batch(spec_btf, threshold, keep_frames=0, min_frames=1):
    """the same for a time-major batch (B, T, F), as tts_speech_frames takes it: two int32 arrays of B entries"""
    out = [speech_frames(np.asarray(u).T, threshold, keep_frames, min_frames) for u in spec_btf]
    return np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32)
