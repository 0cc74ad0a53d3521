"""Mirror of reference audio/features.py (analysis side): STFT and HTK-mel spectrograms on the GPU."""
import numpy as np

from . import default_engine


def linear_scale_spectrogram(wav, n_fft, hop_length=None, win_length=None, engine=None):
    """librosa.stft(wav, n_fft, hop_length, win_length): complex64 (1 + n_fft/2, t)
    (reference audio/features.py:116-145)."""
    eng = engine or default_engine()
    win_length = win_length or n_fft
    hop_length = hop_length or int(win_length // 4)
    wav = np.asarray(wav, dtype=np.float32)
    return eng.stft(wav[None], n_fft, win_length, hop_length).to_host()[0]


def mel_scale_spectrogram(wav, n_fft, sampling_rate, n_mels, fmin, fmax, hop_length, win_length, power, engine=None):
    """reference audio/features.py:5-86: mel (n_mels, t) of abs(stft) ** power, HTK mel scale."""
    eng = engine or default_engine()
    wav = np.asarray(wav, dtype=np.float32)
    lin = eng.stft_magnitude(wav[None], n_fft, win_length, hop_length, power)
    return eng.mel_spectrogram(lin, n_fft, sampling_rate, n_mels, fmin, fmax).to_host()[0]


def calculate_mfccs(mel_spec, sampling_rate, n_mfcc, engine=None):
    """reference audio/features.py:89-113: librosa.feature.mfcc(S=mel_spec, n_mfcc=n_mfcc) -- with S given, the orthonormal DCT-II
    of ``mel_spec`` (n_mels, t) along the mel axis, first ``n_mfcc`` rows: (n_mfcc, t) float32.  No dB conversion happens here:
    pass a dB-scaled spectrogram, as the reference's docstring asks.  ``sampling_rate`` is unused, as in librosa when S is
    given.  The rows are transposed on the host; the transform runs in tts_mfcc."""
    eng = engine or default_engine()
    mel_spec = np.asarray(mel_spec, dtype=np.float32)
    if mel_spec.ndim != 2:
        raise ValueError('calculate_mfccs: mel_spec must be (n_mels, t), got shape {}'.format(mel_spec.shape))
    rows = np.ascontiguousarray(mel_spec.T)[None]
    return np.ascontiguousarray(eng.mfcc(rows, n_mfcc).to_host()[0].T)


def fundamental_frequency(wav, sampling_rate, hop_length, fmin=60.0, fmax=500.0, window=1024, threshold=0.1, want_aperiodicity=False,
                          engine=None):
    """The fundamental frequency of ``wav`` (n,) by YIN, one value per ``hop_length`` samples (frame t sits at sample
    t hop_length, as the frames of the centred STFT do): (1 + n // hop_length,) float32 in Hz, 0 where a frame is unvoiced and
    NaN where its span holds a non-finite sample; with ``want_aperiodicity`` also YIN's normalised difference at the chosen lag.
    No reference counterpart: the reference has no pitch tracker.  The lags searched are max(2, int(sr // fmax)) ..
    ceil(sr / fmin); ``window`` samples enter every sum; a frame is voiced where the normalised difference falls below
    ``threshold``.  Runs in tts_f0 (include/sstts_hip.h has the definition)."""
    eng = engine or default_engine()
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 1 or wav.shape[0] < 1:
        raise ValueError('fundamental_frequency: wav must be a non-empty (n,) array, got shape {}'.format(wav.shape))
    res = eng.f0(wav[None], sampling_rate, hop_length, fmin=fmin, fmax=fmax, window=window, threshold=threshold,
                 want_aperiodicity=want_aperiodicity)
    if not want_aperiodicity:
        out = np.ascontiguousarray(res.to_host()[0])
        res.free()
        return out
    out = tuple(np.ascontiguousarray(r.to_host()[0]) for r in res)
    for r in res:
        r.free()
    return out
