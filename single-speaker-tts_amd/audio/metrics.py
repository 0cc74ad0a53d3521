"""Objective measures of a synthesised spectrogram against its recording.  No reference counterpart: the reference's only
measure is the frame-by-frame L1 loss of ``tacotron.evaluate``, which measures the drift as soon as the free-running decoder
speaks a little faster or slower than the recording.  Mel-cepstral distortion along a dynamic-time-warping path compares the
spectra at the frames that belong together.  The cepstra (tts_mfcc) and the alignment (tts_dtw) run on the device.  Along the
same path, F0 RMSE, voicing error and gross pitch error compare the prosody (tts_f0, tts_f0_compare), which the cepstra do not
see.  ``integrated_loudness`` is the level of a waveform as a listener hears it: ITU-R BS.1770-4 / EBU R 128 (tts_loudness); ``true_peak`` is its
peak between the samples, as delivery specifications state it (tts_true_peak).  ``stoi`` says whether a waveform can be understood
beside a time-aligned clean one: short-time objective intelligibility and its extended form (tts_stoi)."""
import math

import numpy as np

from . import default_engine
from .._hip import STOI_RATE, WM_THRESHOLD, dbtp, resampled_valid, watermark_setting, watermark_zeta
from ..tacotron.params import LJSpeechConstants

MCD_COEFFS = 13


def integrated_loudness(wav, sampling_rate, engine=None):
    """The integrated loudness of one mono waveform (n,) -- or of every row of a batch (B, n) -- in LUFS after ITU-R BS.1770-4 /
    EBU R 128: K-weighting, 400 ms blocks every 100 ms, the absolute gate at -70 LUFS and the relative gate 10 LU under the mean
    of what passed it (``Engine.loudness``).  A float for one waveform, a float64 array (B,) for a batch: -inf for silence or
    less than 400 ms of signal, NaN where a counted block holds a non-finite sample."""
    eng = engine or default_engine()
    wav = wav if hasattr(wav, 'data_ptr') and not isinstance(wav, np.ndarray) else np.asarray(wav, dtype=np.float32)
    out = eng.loudness(wav, sampling_rate)
    return float(out[0]) if len(wav.shape) == 1 else out


def true_peak(wav, engine=None):
    """The true peak of one mono waveform (n,) -- or of every row of a batch (B, n) -- in dBTP after ITU-R BS.1770-4 Annex 2:
    20 log10 of the largest |value| of the 4x oversampled signal (``Engine.true_peak``), never below the sample peak.  A float
    for one waveform, a float64 array (B,) for a batch; -inf for digital silence."""
    eng = engine or default_engine()
    wav = wav if hasattr(wav, 'data_ptr') and not isinstance(wav, np.ndarray) else np.asarray(wav, dtype=np.float32)
    out = dbtp(eng.true_peak(wav))
    return float(out[0]) if len(wav.shape) == 1 else out


def detect_watermark(wav, sampling_rate, key, payload_bits=None, chip=None, chips_per_symbol=None, offsets=64, threshold=WM_THRESHOLD, engine=None):
    """Looks for the carrier of ``key`` (``audio.effects.watermark``, the ``watermark`` of the synthesis calls) in ``wav`` -- one mono
    waveform (n,) or a batch (B, n) at ``sampling_rate``, which may have lost up to ``offsets`` - 1 samples at its front.  Where the
    rate is not the engine's (None: it is), the rows go through ``Engine.resample`` to the engine's rate first, where the carrier
    was laid.  Returns a dict -- a list of dicts for a batch -- of ``offset`` (the samples cut at the front), ``payload`` (the
    bits read), ``zeta`` (``_hip.watermark_zeta``: the score against what P half-normals of the same energy give) and ``detected``
    (zeta above ``threshold``; the default is 1.5 times the largest zeta that wrong keys reached on the oracle).
    The shape parameters left out are the UNTUNED defaults of ``_hip.WM_DEFAULTS``."""
    setting = watermark_setting((key, 0, payload_bits, chip, chips_per_symbol, None))
    eng = engine or default_engine()
    rows = np.asarray(wav, dtype=np.float32)
    single = rows.ndim == 1
    work = None
    if sampling_rate is not None and int(sampling_rate) != eng.sampling_rate:
        work = eng.resample(rows, float(eng.sampling_rate) / float(int(sampling_rate)))
    records = eng.watermark_detect(rows if work is None else work, setting, offsets=offsets)
    if work is not None:
        work.free()
    found = []
    for r in records:
        z = watermark_zeta(r['score'], r['energy'], setting[2])
        found.append(dict(offset=int(r['offset']), payload=int(r['payload']), zeta=z, detected=bool(z > threshold)))
    return found[0] if single else found


STOI_RATE_MIN, STOI_RATE_MAX = STOI_RATE // 4, STOI_RATE * 4   # the resampler's ratios are 0.25 .. 4


def stoi(ref, deg, sampling_rate, extended=False, n_samples=None, engine=None):
    """Short-time objective intelligibility (Taal et al. 2011; ``extended``: ESTOI, Jensen and Taal 2016) of ``deg`` against the
    clean, TIME-ALIGNED ``ref``: one mono waveform (n,) each or batches (B, n) of one shape at ``sampling_rate``, host arrays.
    The figure is defined at 10 000 Hz: at any other rate both signals go through ``Engine.resample`` first (rates outside
    2 500 .. 40 000 Hz are refused: the resampler's ratios are 0.25 .. 4), and ``n_samples`` -- B lengths, None: all n -- become
    the samples the resampler writes for them, int(n * 10000 / sampling_rate).  Returns float64 (B,): about 1 for a copy,
    falling with the damage; NaN for a row with fewer than 30 frames within 40 dB of the reference's loudest, or with a NaN in
    a kept sample.  ``Engine.stoi`` has the frame and segment counts."""
    try:
        ok = int(sampling_rate) == sampling_rate and STOI_RATE_MIN <= sampling_rate <= STOI_RATE_MAX
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError('stoi: the sampling rate must be an integer in {} .. {}, got {!r}'.format(STOI_RATE_MIN, STOI_RATE_MAX, sampling_rate))
    eng = engine or default_engine()
    ref, deg = np.asarray(ref, dtype=np.float32), np.asarray(deg, dtype=np.float32)
    if ref.shape != deg.shape or ref.ndim not in (1, 2) or min(ref.shape) < 1:
        raise ValueError('stoi: ref and deg must be waveforms (n,) or batches (B, n) of one shape, got {} and {}'.format(ref.shape, deg.shape))
    ref, deg = ref.reshape(-1, ref.shape[-1]), deg.reshape(-1, deg.shape[-1])
    ns = None if n_samples is None else np.asarray(n_samples)
    if int(sampling_rate) == STOI_RATE:
        return eng.stoi(ref, deg, n_samples=ns, extended=extended)['value'].copy()
    ratio = float(STOI_RATE) / float(int(sampling_rate))
    r10, d10 = eng.resample(ref, ratio, n_samples=ns), eng.resample(deg, ratio, n_samples=ns)
    try:
        ns10 = None if ns is None else np.array([resampled_valid(n, ratio) for n in ns.tolist()], np.int32)
        if ns is None and resampled_valid(ref.shape[1], ratio) < r10.shape[1]:   # (the buffer is ceil(n ratio) long, the signal int(n ratio))
            ns10 = np.full(ref.shape[0], resampled_valid(ref.shape[1], ratio), np.int32)
        return eng.stoi(r10, d10, n_samples=ns10, extended=extended)['value'].copy()
    finally:
        r10.free()
        d10.free()


def mcd_scale(ref_db, max_db):
    """(sqrt(2) / 2) (|ref_db| + |max_db|): the factor from the Euclidean distance of the cepstra of NORMALISED-dB mel rows to
    mel-cepstral distortion in dB.  De-normalisation is affine, x_db = clip(x, 0, 1) (|ref_db| + |max_db|) - |max_db| + ref_db
    (audio/conversion.py:81-102): its constant moves c0 alone, which is left out, and its factor scales every other coefficient.
    A 20 log10 spectrum is 20 / ln 10 times the natural-log one, so the textbook (10 / ln 10) sqrt(2 sum dc^2) on natural-log
    cepstra is sqrt(2) / 2 times the distance of dB cepstra."""
    return math.sqrt(2.0) / 2.0 * (abs(float(ref_db)) + abs(float(max_db)))


def mel_cepstral_distortion(mel_a, mel_b, n_a=None, n_b=None, n_coeffs=MCD_COEFFS, ref_db=LJSpeechConstants.mel_mag_ref_db,
                            max_db=LJSpeechConstants.mel_mag_max_db, engine=None, want_path=False):
    """Mel-cepstral distortion of B pairs of normalised-dB mel rows, ``mel_a`` (B, Ta, n_mels) against ``mel_b`` (B, Tb, n_mels)
    -- host arrays or device buffers, as the network emits them and the dataset stores them.  ``n_a`` / ``n_b``: B lengths (host
    integers), None: all frames.  Both sides are clipped to [0, 1] as the reference clips before it de-normalises
    (tacotron/inference.py:93-101) and transformed by tts_mfcc to ``n_coeffs`` + 1 orthonormal-DCT coefficients; tts_dtw aligns
    coefficients 1 .. ``n_coeffs`` (c0, the level, is left out), and
        mcd_b = (sqrt(2) / 2) (|ref_db| + |max_db|) cost_b / path_len_b        in dB.
    The orthonormal DCT makes the figure comparable within this project, not with tools of another cepstral convention.
    Returns a dict of host arrays: ``mcd`` (B,) float64, ``cost`` (B,) float64, ``path_len`` (B,) int32 and, with
    ``want_path``, ``path`` (B, Ta + Tb - 1, 2) int32 whose rows behind path_len are (-1, -1)."""
    eng = engine or default_engine()
    if int(n_coeffs) != n_coeffs or n_coeffs < 1:
        raise ValueError('mel_cepstral_distortion: n_coeffs must be an integer >= 1, got {!r}'.format(n_coeffs))
    n_coeffs = int(n_coeffs)
    if len(mel_a.shape) != 3 or len(mel_b.shape) != 3 or mel_a.shape[0] != mel_b.shape[0] or mel_a.shape[2] != mel_b.shape[2]:
        raise ValueError('mel_cepstral_distortion: (B, Ta, n_mels) and (B, Tb, n_mels) rows are needed, got shapes {} and {}'.format(
            tuple(mel_a.shape), tuple(mel_b.shape)))
    if n_coeffs + 1 > mel_a.shape[2]:
        raise ValueError('mel_cepstral_distortion: n_coeffs + 1 = {} coefficients from {} mel bands'.format(n_coeffs + 1, mel_a.shape[2]))
    scale = mcd_scale(ref_db, max_db)
    ca = eng.mfcc(mel_a, n_coeffs + 1, n_frames=n_a, clip01=True)
    cb = eng.mfcc(mel_b, n_coeffs + 1, n_frames=n_b, clip01=True)
    res = eng.dtw(ca, cb, n_a=n_a, n_b=n_b, D=n_coeffs, want_path=want_path, skip=1)
    cost, path_len = res[0].to_host(), res[1].to_host()
    out = dict(mcd=scale * cost / path_len.astype(np.float64), cost=cost, path_len=path_len)
    if want_path:
        out['path'] = res[2].to_host()
    for d in (ca, cb) + tuple(res):
        d.free()
    return out


def f0_errors(f0_a, f0_b, path, engine=None):
    """The F0 and voicing errors of B pairs of F0 tracks, ``f0_a`` (B, Ta) against ``f0_b`` (B, Tb) in Hz -- 0 is unvoiced, side
    b is the recording -- along ``path`` (B, rows, 2), the alignment :func:`mel_cepstral_distortion` returns with ``want_path``
    (rows of (-1, -1) lie behind a path).  Host arrays or device buffers; the reduction runs in tts_f0_compare.  Returns a dict
    of host arrays of B entries:
        f0_rmse_hz         sqrt(sum (fa - fb) ** 2 / n) over the n steps voiced on both sides
        f0_rmse_cents      sqrt(sum (1200 log2(fa / fb)) ** 2 / n) over the same steps
        vuv_error          steps voiced on exactly one side / all steps
        gross_pitch_error  steps voiced on both sides with |fa - fb| > 0.2 fb / steps voiced on both sides
        counts             int32 (B, 5): steps, both voiced, one side voiced, gross pitch errors, NaN steps
    The two RMSEs are NaN where a step holds a NaN (counts[4] > 0) or no step is voiced on both sides; gross_pitch_error is NaN
    where no step is voiced on both sides, vuv_error where the path is empty."""
    eng = engine or default_engine()
    counts_d, sums_d = eng.f0_compare(f0_a, f0_b, path)
    counts, sums = counts_d.to_host(), sums_d.to_host()
    counts_d.free()
    sums_d.free()
    steps, both = counts[:, 0].astype(np.float64), counts[:, 1].astype(np.float64)
    has = (counts[:, 1] > 0) & (counts[:, 4] == 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        rmse_hz = np.where(has, np.sqrt(sums[:, 0] / both), np.nan)
        rmse_cents = np.where(has, np.sqrt(sums[:, 1] / both), np.nan)
        vuv = np.where(steps > 0, counts[:, 2] / steps, np.nan)
        gpe = np.where(both > 0, counts[:, 3] / both, np.nan)
    return dict(f0_rmse_hz=rmse_hz, f0_rmse_cents=rmse_cents, vuv_error=vuv, gross_pitch_error=gpe, counts=counts)
