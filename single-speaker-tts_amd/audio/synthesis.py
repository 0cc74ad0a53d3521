"""Mirror of reference audio/synthesis.py: Griffin-Lim on the GPU.

``spectrogram_to_wav`` (:5-40) and ``griffin_lim_v2`` (:43-125) keep their signatures; two
optional keyword arguments are added because the reference draws its initial phase from the
unseeded global ``np.random`` (:85): ``init_phase`` injects those U[0,1) numbers, ``seed`` draws
them on the device.  A leading batch axis (B, F, T) reconstructs B utterances in one call.

``momentum`` (default 0.0, the reference's loop) is the fast Griffin-Lim momentum of Perraudin, Balazs and Soendergaard
(2013), the ``momentum`` of ``librosa.griffinlim``: the next phases are those of c_i + momentum (c_i - c_{i-1}).  These two
functions state the momentum of every call, as librosa's do: the default 0.0 runs the reference's loop even on an engine
whose ``gl_momentum`` option has been set (``Engine.griffin_lim(momentum=None)`` is the call that follows the option).

``phase_init`` (default 'random', the reference's start) chooses how a call without ``init_phase`` starts: 'estimate' takes
phases estimated from the magnitudes alone (``Engine.phase_estimate``: spectral peaks tracked from frame to frame), from which
the loop reaches the error of 60 iterations in about 12; ``seed`` is then unused.  Stated per call like the momentum; None
follows the engine's ``gl_init`` option.  An explicit ``init_phase`` always wins.

``n_frames`` (B lengths, with a (B, F, T_max) batch) reconstructs utterances of different lengths in one call
(tts_griffin_lim_ragged): utterance b from its first n_frames[b] columns alone -- what lies behind them in ``spectrogram`` and
``init_phase`` reaches nothing -- and the result is a LIST of B arrays of hop (n_frames[b] - 1) samples, each the one a call on
that utterance alone returns."""
import numpy as np

from . import default_engine
from .._hip import momentum_thousandths, phase_init_kwargs, phase_init_value, ragged_frame_counts


def griffin_lim_v2(spectrogram, win_length, hop_length, n_fft, n_iter, init_phase=None, seed=None, engine=None,
                   momentum=0.0, n_frames=None, phase_init='random'):
    """Returns (audio float32 (n,) or (B,n), mse float32); with ``n_frames`` (a list of B arrays, mse float32 (B,))."""
    momentum_thousandths(momentum)   # ValueError outside [0, 1), before an engine is made
    phase_init_value(phase_init)     # likewise
    spec = np.asarray(spectrogram, dtype=np.float32)
    if n_frames is not None:
        if spec.ndim != 3:
            raise ValueError('n_frames needs a (B, F, T_max) batch, got shape {}'.format(spec.shape))
        nf = ragged_frame_counts(n_frames, spec.shape[0], spec.shape[2], hop_length, n_fft)   # ValueError before an engine is made
        eng = engine or default_engine()
        if seed is None and init_phase is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        wav, mse = eng.griffin_lim(spec, n_iter, win_length, hop_length, n_fft, init_phase=init_phase, seed=seed or 0,
                                   momentum=momentum, n_frames=nf, **phase_init_kwargs(eng, phase_init))
        wav, mse = wav.to_host(), mse.to_host()
        wavs = [wav[b, :hop_length * (int(n) - 1)].copy() for b, n in enumerate(nf)]
        return wavs, (None if n_iter == 0 else mse)
    eng = engine or default_engine()
    single = spec.ndim == 2
    if single:
        spec = spec[None]
        if init_phase is not None:
            init_phase = np.asarray(init_phase, dtype=np.float32)[None]
    if seed is None and init_phase is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))   # unseeded, like the reference
    wav, mse = eng.griffin_lim(spec, n_iter, win_length, hop_length, n_fft, init_phase=init_phase, seed=seed or 0,
                               momentum=momentum, **phase_init_kwargs(eng, phase_init))
    wav, mse = wav.to_host(), mse.to_host()
    if n_iter == 0:
        return (wav[0], None) if single else (wav, None)
    return (wav[0], mse[0]) if single else (wav, mse)


def spectrogram_to_wav(mag, win_length, hop_length, n_fft, n_iter, init_phase=None, seed=None, engine=None, momentum=0.0,
                       n_frames=None, phase_init='random'):
    """reference audio/synthesis.py:5-40; with ``n_frames`` a list of per-utterance waveforms."""
    wav, _ = griffin_lim_v2(mag, win_length=win_length, hop_length=hop_length, n_fft=n_fft, n_iter=n_iter,
                            init_phase=init_phase, seed=seed, engine=engine, momentum=momentum, n_frames=n_frames, phase_init=phase_init)
    if n_frames is not None:
        return [w.astype(np.float32) for w in wav]
    return wav.astype(np.float32)
