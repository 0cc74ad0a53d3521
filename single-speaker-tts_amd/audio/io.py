"""Mirror of reference audio/io.py: ``save_wav`` (:33-53, float32 WAV, optional peak normalisation) and ``load_wav``
(:8-30, librosa.core.load of a RIFF/WAVE file at its native rate; standard library and numpy only).  ``resample`` is the
resampler librosa.core.load runs for another rate, librosa.core.resample, on the GPU (tts_resample); ``load_wav`` does not call it.

librosa.output.write_wav(path, y.astype(float32), sr, norm=True) = util.normalize(y, norm=inf)
then scipy.io.wavfile.write of float32 samples (WAVE_FORMAT_IEEE_FLOAT).  The normalisation runs
on the GPU (tts_peak_normalize); the container is written with the standard library."""
import struct

import numpy as np

from . import default_engine


def _write_float32_wav(path, data, sampling_rate):
    data = np.ascontiguousarray(data, dtype='<f4')
    if data.ndim == 2:          # (2, n) stereo as the reference documents -> interleave
        channels = data.shape[0]
        data = np.ascontiguousarray(data.T)
    else:
        channels = 1
    nbytes = data.nbytes
    with open(path, 'wb') as f:
        # RIFF / fmt (IEEE float, 18-byte fmt chunk) / fact / data -- what scipy.io.wavfile emits
        fmt = struct.pack('<HHIIHHH', 3, channels, sampling_rate, sampling_rate * channels * 4, channels * 4, 32, 0)
        fact = struct.pack('<I', data.shape[0])
        riff_size = 4 + (8 + len(fmt)) + (8 + len(fact)) + (8 + nbytes)
        f.write(b'RIFF' + struct.pack('<I', riff_size) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<I', len(fmt)) + fmt)
        f.write(b'fact' + struct.pack('<I', len(fact)) + fact)
        f.write(b'data' + struct.pack('<I', nbytes))
        f.write(data.tobytes())


def save_wav(wav_path, wav, sampling_rate, norm=False, engine=None):
    """reference audio/io.py:33-53."""
    wav = np.asarray(wav).astype(np.float32)
    if norm:
        eng = engine or default_engine()
        flat = wav.reshape(1, -1)            # inf-norm over the whole array (axis=None)
        wav = eng.peak_normalize(eng.to_device(flat)).to_host().reshape(wav.shape)
    _write_float32_wav(wav_path, wav, sampling_rate)


_PCM, _IEEE_FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def _read_wav(path):
    """-> (format tag, channels, rate, bits, raw data bytes) of a RIFF/WAVE file."""
    with open(path, 'rb') as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b'RIFF' or blob[8:12] != b'WAVE':
        raise ValueError('{}: not a RIFF/WAVE file (format tag {!r})'.format(path, blob[:4]))
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack('<I', blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b'fmt ':
            if len(body) < 16:
                raise ValueError('{}: truncated fmt chunk'.format(path))
            tag, channels, rate, _, _, bits = struct.unpack('<HHIIHH', body[:16])
            if tag == _EXTENSIBLE and len(body) >= 26:
                tag = struct.unpack('<H', body[24:26])[0]   # first two bytes of the sub-format GUID
            fmt = (tag, channels, rate, bits)
        elif cid == b'data':
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError('{}: no {} chunk'.format(path, 'fmt' if fmt is None else 'data'))
    return fmt + (data,)


def resample(wav, orig_sr, target_sr, engine=None):
    """librosa 0.6 librosa.core.resample(wav, orig_sr, target_sr, res_type='kaiser_best', fix=True, scale=False) of a mono
    waveform (n,): resampy's windowed-sinc interpolator computed by tts_resample, zero-padded to ceil(n * target_sr / orig_sr)
    samples; equal rates return ``wav`` itself, as librosa does.  The ratio target_sr / orig_sr must lie in [0.25, 4]."""
    if orig_sr == target_sr:
        return wav
    wav = np.asarray(wav)
    if wav.ndim != 1 or wav.shape[0] < 1:
        raise ValueError('resample: a mono waveform (n,) is needed, got shape {}'.format(wav.shape))
    ratio = float(target_sr) / orig_sr
    eng = engine or default_engine()
    out = eng.resample(wav.astype(np.float32), ratio)
    y = out.to_host()
    out.free()
    return np.ascontiguousarray(y, dtype=wav.dtype if wav.dtype.kind == 'f' else np.float32)


def load_wav(wav_path, sampling_rate=None, offset=0.0, duration=None):
    """reference audio/io.py:8-30: librosa.core.load(path, sr=None, offset, duration) of a RIFF/WAVE file ->
    (float32 mono samples, native rate).  PCM 8 (unsigned), 16, 24, 32 bit and IEEE float32 / float64; integers scaled by
    1 / 2 ** (bits - 1), channels averaged; offset / duration in seconds at int(round(sr * x)) samples.  Resampling is out of
    scope: any `sampling_rate` other than None or the native rate raises NotImplementedError."""
    tag, channels, rate, bits, raw = _read_wav(wav_path)
    if sampling_rate is not None and int(sampling_rate) != rate:
        raise NotImplementedError('load_wav: resampling {} Hz -> {} Hz is not supported'.format(rate, sampling_rate))
    if channels < 1:
        raise ValueError('{}: {} channels'.format(wav_path, channels))
    if tag == _PCM and bits in (8, 16, 24, 32):
        width = bits // 8
        n = len(raw) // (width * channels)
        raw = raw[:n * width * channels]
        if bits == 8:
            x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0)
        elif bits == 24:
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float32)
        else:
            x = np.frombuffer(raw, dtype='<i{}'.format(width)).astype(np.float32)
        x = x * np.float32(1.0 / float(1 << (bits - 1)))
    elif tag == _IEEE_FLOAT and bits in (32, 64):
        width = bits // 8
        n = len(raw) // (width * channels)
        x = np.frombuffer(raw[:n * width * channels], dtype='<f{}'.format(width)).astype(np.float32)
    else:
        raise ValueError('{}: unsupported WAV format tag {} with {} bits per sample'.format(wav_path, tag, bits))
    x = x.reshape(-1, channels)
    y = x[:, 0].copy() if channels == 1 else np.mean(x, axis=1, dtype=np.float32)
    start = int(round(rate * offset))
    stop = None if duration is None else start + int(round(rate * duration))
    return np.ascontiguousarray(y[start:stop], dtype=np.float32), rate
