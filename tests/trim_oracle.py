"""Float64 numpy restatement of librosa 0.6 ``effects.trim`` and of the reference's feature pipeline (datasets/lj_speech.py:
106-156 load_audio), composed from ``oracle.audio_oracle`` (a plain helper module, imported like conftest's helpers).

trim: reflect-pad y by frame_length // 2, frames k = 0 .. n // hop, mse_k = mean(frame ** 2); frame k is non-silent iff
10 log10(max(1e-10, mse_k)) - 10 log10(max(1e-10, max mse)) > -top_db; start = first * hop, end = min(n, (last + 1) * hop).

Non-finite samples are decided as numpy decides them: ``mse.max()`` and ``np.maximum`` carry a NaN, so one NaN sample makes the
reference level NaN and every comparison false -- no frame is non-silent and the bounds are (0, 0).  A +-Inf sample ends there
too: its frames are Inf - Inf = NaN against the reference, all others -Inf."""
import numpy as np

from oracle import audio_oracle as A


def frame_power_db(y, frame_length=2048, hop_length=512):
    """(mse per frame, its dB against the loudest frame), float64."""
    y = np.asarray(y, dtype=np.float64)
    yp = np.pad(y, frame_length // 2, mode='reflect')
    n_frames = 1 + len(y) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n_frames)[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        mse = np.mean(yp[idx] ** 2, axis=1)
        db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))   # numpy's own max: NaN stays
    return mse, db


def trim_bounds(y, top_db=60, frame_length=2048, hop_length=512):
    _, db = frame_power_db(y, frame_length, hop_length)
    nz = np.flatnonzero(db > -top_db)
    if len(nz) == 0:
        return 0, 0
    return int(nz[0] * hop_length), int(min(len(y), (nz[-1] + 1) * hop_length))


def threshold_margin(y, top_db=60, frame_length=2048, hop_length=512):
    """Smallest |dB - (-top_db)| over the frames: how far the decision is from the threshold."""
    _, db = frame_power_db(y, frame_length, hop_length)
    return float(np.min(np.abs(db + top_db)))


def reduction_pad(mel, lin, r):
    """reference dataset_helper.py:357-401 on (T, n_mels), (T, F)."""
    T = mel.shape[0]
    if T % r:
        pad = r - T % r
        mel = np.pad(mel, [[0, pad], [0, 0]], mode='constant')
        lin = np.pad(lin, [[0, pad], [0, 0]], mode='constant')
    return mel.reshape(-1, mel.shape[1] * r), lin.reshape(-1, lin.shape[1] * r)


def features(y, sr=22050, n_fft=2048, win=1102, hop=275, n_mels=80, fmin=0.0, fmax=8000.0, consts=(6.02, 99.89, 35.66, 100.0),
             normalize=True, r=5, trim=True, top_db=60):
    """(mel (T_red, n_mels r), lin (T_red, F r)) in float64 as load_audio computes them."""
    y = np.asarray(y, dtype=np.float32)
    if trim:
        s, e = trim_bounds(y, top_db)
        y = y[s:e]
    spec = A.stft(y.astype(np.float64), n_fft, hop, win, dtype=np.complex128)    # (F, T)
    mag = np.abs(spec)
    mel = A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax) @ mag
    lin_db = A.magnitude_to_decibel(mag.T)
    mel_db = A.magnitude_to_decibel(mel.T)
    if normalize:
        mel_db = A.normalize_decibel(mel_db, consts[0], consts[1])
        lin_db = A.normalize_decibel(lin_db, consts[2], consts[3])
    return reduction_pad(mel_db, lin_db, r)
