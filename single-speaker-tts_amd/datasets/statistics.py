"""Mirror of reference datasets/statistics.py:11-98: the dB statistics the feature normalisation constants come from.

The spectrograms are computed by tts_extract_features (no trim, no normalisation: raw dB rows, n_fft 1024, hop 256,
window 1024, 80 HTK mel bands over 0 .. sr // 2); the per-file min / max are taken on the host.  The reconstruction-error
statistics and plots of the reference module (:101-258) are out of scope."""
import numpy as np

from ..audio import default_engine
from ..audio.io import load_wav

N_FFT = 1024


def _params(engine, sampling_rate):
    return engine.feature_params(n_fft=N_FFT, win_length=N_FFT, hop_length=N_FFT // 4, sampling_rate=int(sampling_rate),
                                 n_mels=80, fmin=0.0, fmax=float(sampling_rate // 2), normalize=0, reduction=1, trim=0)


def _stats(mel_db, lin_db):
    return np.array([np.min(lin_db), np.max(lin_db), np.min(mel_db), np.max(mel_db)])


def decibel_statistics(wav, sampling_rate, engine=None):
    """reference :11-63: np.array([min(linear_db), max(linear_db), min(mel_db), max(mel_db)]) of one recording."""
    eng = engine or default_engine()
    mel_db, lin_db = eng.extract_features([np.asarray(wav, dtype=np.float32)], _params(eng, sampling_rate))[0]
    return _stats(mel_db, lin_db)


def collect_decibel_statistics(path_listing, batch_size=32, engine=None):
    """reference :66-98: the four statistics averaged over the files (recordings of one rate are batched together)."""
    eng = engine or default_engine()
    paths = [p.decode() if isinstance(p, bytes) else p for p in path_listing]
    stats = np.zeros(4)
    for i in range(0, len(paths), max(1, int(batch_size))):
        loaded = [load_wav(p) for p in paths[i:i + batch_size]]
        for sr in sorted({sr for _, sr in loaded}):
            wavs = [w for w, r in loaded if r == sr]
            for mel_db, lin_db in eng.extract_features(wavs, _params(eng, sr)):
                stats += _stats(mel_db, lin_db)
    stats /= len(paths)
    return stats
