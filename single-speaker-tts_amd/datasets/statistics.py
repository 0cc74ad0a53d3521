"""Mirror of reference datasets/statistics.py:11-98: the dB statistics the feature normalisation constants come from.

The spectrograms are computed by tts_extract_features (no trim, no normalisation: raw dB rows, n_fft 1024, hop 256,
window 1024, 80 HTK mel bands over 0 .. sr // 2); the per-file min / max are taken on the host.

``collect_reconstruction_error`` is the reference's :146-187 -- |STFT| of every recording followed by Griffin-Lim, the mean
of the last iteration's mse -- as ragged batches: one tts_griffin_lim_ragged call reconstructs ``batch_size`` recordings of
different lengths.  ``collect_loudness`` has no reference counterpart: the integrated loudness (ITU-R BS.1770-4, tts_loudness)
of every recording and its spread over the corpus, which the dB statistics do not show.  ``collect_intelligibility`` has none
either: STOI / ESTOI (tts_stoi) of every recording's Griffin-Lim reconstruction against the recording itself -- whether what the
vocoder makes of a perfect spectrogram can be understood, beside the spectrogram mse that says how well it converged.  The duration statistics and the plots of the reference module (:101-143, :190-258) are out of scope."""
import numpy as np

from ..audio import default_engine
from ..audio.conversion import ms_to_samples
from ..audio.io import load_wav
from ..audio.metrics import stoi
from ..audio.synthesis import griffin_lim_v2

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


def collect_loudness(path_listing, batch_size=32, engine=None):
    """The integrated loudness of every recording, ``batch_size`` files at a time: those of one sampling rate are measured in
    ONE ragged ``Engine.loudness`` call, so the padding is neither read nor able to change a result.  Returns a dict: ``lufs``,
    float64 (files,) in the order of the listing (-inf: silent or shorter than 400 ms), and ``min`` / ``max`` / ``mean`` /
    ``std`` in LUFS over the recordings with a finite figure (NaN when there is none), ``measured`` their count."""
    eng = engine or default_engine()
    paths = [p.decode() if isinstance(p, bytes) else p for p in path_listing]
    lufs = np.full(len(paths), np.nan)
    step = max(1, int(batch_size))
    for i in range(0, len(paths), step):
        loaded = [load_wav(p) for p in paths[i:i + step]]
        for sr in sorted({r for _, r in loaded}):
            group = [k for k, (_, r) in enumerate(loaded) if r == sr]
            lens = np.array([len(loaded[k][0]) for k in group], dtype=np.int32)
            rows = np.zeros((len(group), int(lens.max())), dtype=np.float32)
            for row, k in enumerate(group):
                rows[row, :lens[row]] = np.asarray(loaded[k][0], dtype=np.float32)
            lufs[[i + k for k in group]] = eng.loudness(rows, int(sr), n_samples=lens)
    finite = lufs[np.isfinite(lufs)]
    nan = float('nan')
    return dict(lufs=lufs, measured=int(finite.size), min=float(finite.min()) if finite.size else nan,
                max=float(finite.max()) if finite.size else nan, mean=float(finite.mean()) if finite.size else nan,
                std=float(finite.std()) if finite.size else nan)


RECONSTRUCTION_N_FFT = 2048      # reference :149
RECONSTRUCTION_WIN_MS = 50.0     # :152
RECONSTRUCTION_HOP_MS = 12.5     # :155


def _padded_magnitudes(eng, wavs, n_fft, win, hop):
    """|STFT| of every recording (Engine.stft_magnitude, recordings of one length in one call) packed into a zero-padded
    (B, F, T_max) array; returns it with the frame counts 1 + n // hop."""
    frames = [1 + len(w) // hop for w in wavs]
    mag = np.zeros((len(wavs), 1 + n_fft // 2, max(frames)), dtype=np.float32)
    by_len = {}
    for i, w in enumerate(wavs):
        by_len.setdefault(len(w), []).append(i)
    for n, idx in sorted(by_len.items()):
        m = eng.stft_magnitude(np.stack([np.asarray(wavs[i], dtype=np.float32) for i in idx]), n_fft, win, hop)
        m = m.to_host() if hasattr(m, 'to_host') else np.asarray(m)
        for k, i in enumerate(idx):
            mag[i, :, :frames[i]] = m[k]
    return mag, frames


def collect_reconstruction_error(path_listing, n_iters, batch_size=32, seed=None, engine=None, init_phases=None):
    """reference :146-187: the mean over the files of the Griffin-Lim reconstruction error after ``n_iters`` iterations, at
    n_fft 2048 with a 50 ms window and a 12.5 ms hop (``ms_to_samples`` of each file's sampling rate).  Printed and returned.

    The recordings are taken ``batch_size`` files at a time; those of one sampling rate are sorted by length and
    reconstructed in ONE ragged Griffin-Lim call (``griffin_lim_v2(..., n_frames=...)``), so the padding is neither computed
    nor able to change a result.  ``seed`` seeds the initial phases (None: unseeded, like the reference);
    ``init_phases`` (a test hook, as ``griffin_lim_v2``'s ``init_phase``) maps a path to its (F, T) array of U[0, 1) numbers."""
    eng = engine or default_engine()
    paths = [p.decode() if isinstance(p, bytes) else p for p in path_listing]
    n_fft = RECONSTRUCTION_N_FFT
    print('Collecting reconstruction statistics for {} files ...'.format(len(paths)))
    mse_errors = []
    step = max(1, int(batch_size))
    for i in range(0, len(paths), step):
        chunk = paths[i:i + step]
        loaded = [load_wav(p) for p in chunk]
        for sr in sorted({r for _, r in loaded}):
            win = ms_to_samples(RECONSTRUCTION_WIN_MS, sampling_rate=sr)
            hop = ms_to_samples(RECONSTRUCTION_HOP_MS, sampling_rate=sr)
            group = sorted((k for k, (_, r) in enumerate(loaded) if r == sr), key=lambda k: len(loaded[k][0]))
            mag, frames = _padded_magnitudes(eng, [loaded[k][0] for k in group], n_fft, win, hop)
            init = None
            if init_phases is not None:
                init = np.zeros(mag.shape, dtype=np.float32)
                for row, k in enumerate(group):
                    init[row, :, :frames[row]] = np.asarray(init_phases[chunk[k]], dtype=np.float32)
            batch_seed = None if seed is None else int(seed) + i
            _, mse = griffin_lim_v2(mag, win_length=win, hop_length=hop, n_fft=n_fft, n_iter=n_iters, init_phase=init,
                                    seed=batch_seed, engine=eng, n_frames=frames)
            mse_errors.extend(float(m) for m in (mse if mse is not None else np.zeros(len(group))))
    total_mse = sum(mse_errors) / len(mse_errors)
    print('Dataset MSE with {} iterations: {}'.format(n_iters, total_mse))
    return total_mse


def collect_intelligibility(path_listing, n_iters, batch_size=32, seed=None, momentum=0.0, phase_init=None, extended=False, engine=None):
    """STOI (``extended``: ESTOI) of every recording's Griffin-Lim reconstruction after ``n_iters`` iterations against the
    recording itself: |STFT| at the settings of ``collect_reconstruction_error`` (n_fft 2048, a 50 ms window, a 12.5 ms hop),
    the same grouping -- ``batch_size`` files at a time, those of one sampling rate sorted by length and reconstructed in ONE
    ragged Griffin-Lim call -- and the same seeding (``seed`` + the batch's first index; None: unseeded).  ``momentum`` and
    ``phase_init`` (None: 'random') are ``griffin_lim_v2``'s.  The two signals are time-aligned by construction and compared
    over the samples both hold (the reconstruction ends at the last whole hop); ``audio.metrics.stoi`` brings them to 10 kHz.
    Returns a dict: ``stoi``, float64 (files,) in the order of the listing (NaN: fewer than 30 frames within 40 dB of the
    recording's loudest), and ``min`` / ``max`` / ``mean`` / ``std`` over the recordings with a finite figure (NaN when there is
    none), ``measured`` their count."""
    eng = engine or default_engine()
    paths = [p.decode() if isinstance(p, bytes) else p for p in path_listing]
    n_fft = RECONSTRUCTION_N_FFT
    values = np.full(len(paths), np.nan)
    step = max(1, int(batch_size))
    for i in range(0, len(paths), step):
        loaded = [load_wav(p) for p in paths[i:i + step]]
        for sr in sorted({r for _, r in loaded}):
            win = ms_to_samples(RECONSTRUCTION_WIN_MS, sampling_rate=sr)
            hop = ms_to_samples(RECONSTRUCTION_HOP_MS, sampling_rate=sr)
            group = sorted((k for k, (_, r) in enumerate(loaded) if r == sr), key=lambda k: len(loaded[k][0]))
            mag, frames = _padded_magnitudes(eng, [loaded[k][0] for k in group], n_fft, win, hop)
            batch_seed = None if seed is None else int(seed) + i
            wavs, _ = griffin_lim_v2(mag, win_length=win, hop_length=hop, n_fft=n_fft, n_iter=n_iters, seed=batch_seed, engine=eng,
                                     momentum=momentum, n_frames=frames, phase_init='random' if phase_init is None else phase_init)
            lens = np.array([min(len(loaded[k][0]), len(w)) for k, w in zip(group, wavs)], dtype=np.int32)
            ref = np.zeros((len(group), int(lens.max())), dtype=np.float32)
            deg = np.zeros_like(ref)
            for row, k in enumerate(group):
                ref[row, :lens[row]] = np.asarray(loaded[k][0], dtype=np.float32)[:lens[row]]
                deg[row, :lens[row]] = wavs[row][:lens[row]]
            values[[i + k for k in group]] = stoi(ref, deg, int(sr), extended=extended, n_samples=lens, engine=eng)
    finite = values[np.isfinite(values)]
    nan = float('nan')
    return dict(stoi=values, measured=int(finite.size), min=float(finite.min()) if finite.size else nan,
                max=float(finite.max()) if finite.size else nan, mean=float(finite.mean()) if finite.size else nan,
                std=float(finite.std()) if finite.size else nan)
