"""Mirror of reference audio/effects.py: silence trimming and cropping.

``trim_silence`` is librosa.effects.trim (librosa 0.6: frame length 2048, hop 512, reference power = the loudest frame)
computed by tts_trim_bounds on the GPU.

``time_stretch`` and ``pitch_shift`` raise NotImplementedError here.  The reference's time_stretch (:46-88) is an STFT, the
librosa phase vocoder, np.abs and Griffin-Lim; on this path that is ``Engine.time_stretch(wavs, rate)`` (device calls:
tts_stft_magnitude, tts_stretch_magnitudes, tts_griffin_lim), and the speaking rate of synthesis is the ``speaking_rate``
argument of the synthesis calls (tts_set_speaking_rate), which stretches the magnitudes a call already holds ahead of its one
Griffin-Lim.  ``pitch_shift`` (:9-43) is that time_stretch at 2 ** -octaves followed by librosa's resampler (resampy's
'kaiser_best' windowed sinc) back to the input's length; on this path that is ``Engine.pitch_shift(wavs, sampling_rate, octaves)``
(``Engine.time_stretch``, then ``Engine.resample``: tts_resample), and the pitch of synthesis is the ``pitch`` argument of the
synthesis calls (tts_set_pitch), which stretches the call's magnitudes and resamples what its one Griffin-Lim made.

``normalize_loudness`` has no reference counterpart (the reference's only level control is the peak normalisation of save_wav):
one gain takes a waveform to a target integrated loudness after ITU-R BS.1770-4 (tts_loudness_normalize); the loudness of
synthesis is the ``loudness`` argument of the synthesis calls (tts_set_loudness).  ``limit`` is the look-ahead peak limiter behind
it (tts_limit; the ``limiter`` argument of the synthesis calls, tts_set_limiter).  ``equalize`` shapes the spectrum with a cascade
of second-order sections (tts_equalize; the ``equalizer`` argument of the synthesis calls, tts_set_equalizer), and ``compress``
lowers the crest factor with a feed-forward peak compressor (tts_compress; the ``compressor`` argument, tts_set_compressor).
``watermark`` adds a keyed spread-spectrum carrier under the local envelope (tts_watermark_embed; the ``watermark`` argument,
tts_set_watermark); ``audio.metrics.detect_watermark`` looks for it."""
import numpy as np

from . import default_engine
from .conversion import ms_to_samples
from .._hip import compressor_params, compressor_setting, equalizer_sections, equalizer_setting, limiter_lookahead, watermark_setting


def pitch_shift(wav, sampling_rate, octaves, preserve_formants=False, n_iter=25, seed=0, engine=None):
    """With ``preserve_formants`` (no reference counterpart): ``wav`` -- one mono waveform (n,) or a uniform batch (B, n) -- with its
    pitch moved by ``octaves`` and its spectral envelope left where it is, at the same length (``Engine.pitch_shift(..,
    preserve_formants=True)``: STFT magnitude, ``shift_magnitudes``, Griffin-Lim).  Returns a float32 host array of the input's
    shape.  Without it: the reference's resampling form, which is out of scope here."""
    if not preserve_formants:
        raise NotImplementedError('pitch_shift (librosa resampling, reference audio/effects.py:9-43) is out of scope')   # see Engine.pitch_shift
    eng = engine or default_engine()
    out = eng.pitch_shift(np.asarray(wav, dtype=np.float32), sampling_rate, octaves, n_iter=n_iter, seed=seed, preserve_formants=True)
    host = out.to_host()
    out.free()
    return host


def time_stretch(wav, rate):
    raise NotImplementedError('time_stretch (librosa phase vocoder, reference audio/effects.py:46-88) is out of scope')


def normalize_loudness(wav, sampling_rate, target_lufs=-23.0, max_peak=1.0, engine=None):
    """``wav`` -- one mono waveform (n,) or a batch (B, n) -- scaled to ``target_lufs`` of integrated loudness (ITU-R BS.1770-4),
    each utterance by one gain that leaves no sample beyond ``max_peak`` (``Engine.loudness_normalize``).  A waveform that is
    silent, shorter than 400 ms or holds a non-finite sample in a counted block comes back as it is.  Returns a float32 host
    array of the input's shape."""
    eng = engine or default_engine()
    out, _gains = eng.loudness_normalize(np.asarray(wav, dtype=np.float32), sampling_rate, target_lufs, max_peak)
    host = out.to_host()
    out.free()
    return host


def limit(wav, ceiling, sampling_rate=None, lookahead_ms=5.0, true_peak=True, engine=None):
    """``wav`` -- one mono waveform (n,) or a batch (B, n) -- through the look-ahead peak limiter (``Engine.limit``): no finite
    sample of the result is above ``ceiling`` (linear, e.g. 10 ** (-1 / 20)), the gain falls over ``lookahead_ms`` ahead of a peak and
    recovers over as long behind it, and a waveform that never reaches the ceiling comes back as its own bits.  ``true_peak``:
    the ceiling is held against the 4x interpolated peaks (``metrics.true_peak``), not the samples alone.  ``sampling_rate``
    turns the look-ahead into samples (None: the engine's).  Returns a float32 host array of the input's shape."""
    eng = engine or default_engine()
    L = limiter_lookahead('limit', lookahead_ms, eng.sampling_rate if sampling_rate is None else sampling_rate)
    out, _stats = eng.limit(np.asarray(wav, dtype=np.float32), ceiling, L, 4 if true_peak else 1)
    host = out.to_host()
    out.free()
    return host


def equalize(wav, sampling_rate, equalizer, engine=None):
    """``wav`` -- one mono waveform (n,) or a batch (B, n) -- through a cascade of up to 8 second-order sections
    (``Engine.equalize``).  ``equalizer``: a profile name -- 'telephony', 'small-speaker', 'rumble', 'bright', 'warm'; every preset is
    untuned --, a list of ``(kind, f0_hz[, q[, gain_db]])`` sections or an (S, 5) array of sections b0 b1 b2 a1 a2; a profile
    or a design is made at ``sampling_rate`` (None: the engine's), and a corner that does not fit under 0.49 of it is a
    ValueError.  The length does not change: the group delay of a few samples stays in.  Returns a float32 host array of the
    input's shape."""
    setting = equalizer_setting(equalizer)
    if setting is None:
        raise ValueError('equalize: an equalizer is needed')
    eng = engine or default_engine()
    out = eng.equalize(np.asarray(wav, dtype=np.float32), equalizer_sections(setting, eng.sampling_rate if sampling_rate is None else int(sampling_rate)))
    host = out.to_host()
    out.free()
    return host


def compress(wav, sampling_rate, compressor, engine=None):
    """``wav`` -- one mono waveform (n,) or a batch (B, n) -- through a feed-forward peak compressor (``Engine.compress``).
    ``compressor``: a profile name -- 'speech', 'telephony', 'small-speaker'; every preset is untuned -- or ``(threshold_db, ratio[,
    knee_db[, attack_ms[, release_ms[, makeup_db]]]])``; the attack and release become coefficients at ``sampling_rate`` (None: the
    engine's).  The length does not change.  Returns a float32 host array of the input's shape."""
    setting = compressor_setting(compressor)
    if setting is None:
        raise ValueError('compress: a compressor is needed')
    eng = engine or default_engine()
    params = compressor_params(setting, eng.sampling_rate if sampling_rate is None else int(sampling_rate))
    out = eng.compress(np.asarray(wav, dtype=np.float32), ('params', params))
    host = out.to_host()
    out.free()
    return host


def watermark(wav, key, payload=0, payload_bits=None, chip=None, chips_per_symbol=None, strength=None, engine=None):
    """``wav`` -- one mono waveform (n,) or a batch (B, n) -- with the keyed carrier of ``Engine.watermark_embed`` added under its
    local envelope; the carrier starts at every row's first sample.  ``key``: an integer in 0 .. 2^64 - 1; ``payload``: its low
    ``payload_bits`` bits travel.  What is left out is ``_hip.WM_DEFAULTS`` -- 16 bits, 8 samples a chip, 64 chips a symbol, a
    strength of 0.02 of the envelope: UNTUNED, nobody has listened.  The length does not change.  Returns a float32 host array of
    the input's shape."""
    setting = watermark_setting((key, payload, payload_bits, chip, chips_per_symbol, strength))
    eng = engine or default_engine()
    out = eng.watermark_embed(np.asarray(wav, dtype=np.float32), setting)
    host = out.to_host()
    out.free()
    return host


def trim_silence(wav, threshold_db=40, ref=np.max, engine=None):
    """reference :188-215: (wav[start:end], np.array([start, end])) of librosa.effects.trim(wav, threshold_db, ref).
    Only ``ref=np.max`` (the reference's default) is supported."""
    if ref is not np.max:
        raise NotImplementedError('trim_silence: only ref=np.max is supported')
    eng = engine or default_engine()
    wav = np.asarray(wav)
    start, end = (int(v) for v in eng.trim_bounds([wav.astype(np.float32)], 2048, 512, float(threshold_db))[0])
    return wav[start:end], np.array([start, end])


def crop_silence_left(wav, sampling_rate, length_ms, safe_crop=True):
    """reference :91-136: (wav[n_cropped:], n_cropped), n_cropped = min(samples(length_ms), leading silence) when
    safe_crop."""
    assert (length_ms > 0), 'Crop length must be greater 0.'
    samples = ms_to_samples(length_ms, sampling_rate)
    assert (samples < len(wav)), 'Crop length can not be greater than the total wav length.'
    if safe_crop:
        _, non_silence_region = trim_silence(wav)
        samples = min(samples, non_silence_region[0])
    return wav[samples:], samples


def crop_silence_right(wav, sampling_rate, length_ms, safe_crop=True):
    """reference :139-185: (wav[:-n_cropped], n_cropped).  As in the reference, n_cropped = 0 returns an empty array."""
    assert (length_ms > 0), 'Crop length must be greater 0.'
    samples = ms_to_samples(length_ms, sampling_rate)
    assert (samples < len(wav)), 'Crop length can not be greater than the total wav length.'
    if safe_crop:
        _, non_silence_region = trim_silence(wav)
        samples = min(samples, len(wav) - non_silence_region[1])
    return wav[:-samples], samples


def silence_interval_from_spectrogram(mag_spec_db, threshold_db, ref=np.max):
    """reference :218-233 (host numpy): first and last frame (column) whose reference dB exceeds threshold_db, or None."""
    ref_trim_spec_db = ref(mag_spec_db, axis=0)
    nonzero = np.flatnonzero(np.array(ref_trim_spec_db > threshold_db, dtype=np.int32))
    if len(nonzero) == 0:
        return None
    return np.min(nonzero), np.max(nonzero)
