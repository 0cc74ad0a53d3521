"""Mirror of reference audio/io.py: ``save_wav`` (:33-53, float32 WAV, optional peak normalisation) and ``load_wav``
(:8-30, librosa.core.load of a RIFF/WAVE file at its native rate; standard library and numpy only).  ``resample`` is the
resampler librosa.core.load runs for another rate, librosa.core.resample, on the GPU (tts_resample); ``load_wav`` does not call it.

librosa.output.write_wav(path, y.astype(float32), sr, norm=True) = util.normalize(y, norm=inf)
then scipy.io.wavfile.write of float32 samples (WAVE_FORMAT_IEEE_FLOAT).  The normalisation runs
on the GPU (tts_peak_normalize); the container is written with the standard library.

Beyond the reference: ``save_wav(encoding=...)`` writes 16-bit PCM, 8-bit PCM and G.711 mu-law / A-law files, encoded on the GPU
(tts_encode: TPDF dither, round to nearest even, saturation), and ``load_wav`` reads G.711 files through the decode tables."""
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


_PCM, _IEEE_FLOAT, _ALAW, _MULAW, _EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
# encoding -> (format tag, numpy type of a stored code)
ENCODINGS = {'float32': (_IEEE_FLOAT, np.float32), 'pcm16': (_PCM, np.int16), 'pcm8': (_PCM, np.uint8), 'mulaw': (_MULAW, np.uint8),
             'alaw': (_ALAW, np.uint8)}


def _write_coded_wav(path, codes, sampling_rate, tag):
    """int16 or uint8 codes, (n,) or (channels, n), as a RIFF/WAVE file: PCM (tag 1) with the 16-byte fmt chunk, G.711 (tags 6 and
    7) with the 18-byte fmt chunk and a fact chunk, as non-PCM formats must have them"""
    if codes.ndim == 2:
        channels = codes.shape[0]
        codes = np.ascontiguousarray(codes.T)
    else:
        channels = 1
    width = codes.dtype.itemsize
    data = codes.astype(codes.dtype.newbyteorder('<')).tobytes()
    fmt = struct.pack('<HHIIHH', tag, channels, sampling_rate, sampling_rate * channels * width, channels * width, 8 * width)
    fact = b''
    if tag != _PCM:
        fmt += struct.pack('<H', 0)
        fact = b'fact' + struct.pack('<II', 4, codes.shape[0])
    pad = b'\x00' * (len(data) & 1)
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 4 + (8 + len(fmt)) + len(fact) + (8 + len(data) + len(pad))) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<I', len(fmt)) + fmt + fact)
        f.write(b'data' + struct.pack('<I', len(data)) + data + pad)


def save_wav(wav_path, wav, sampling_rate, norm=False, engine=None, encoding='float32', dither=True):
    """reference audio/io.py:33-53 with the default ``encoding`` 'float32': the reference's bytes.  'pcm16', 'pcm8', 'mulaw' and
    'alaw' encode the (normalised) float samples on the GPU (``Engine.encode``: TPDF dither unless ``dither`` is false, seed 0,
    channel c dithered as row c) and write 16-bit PCM, unsigned 8-bit PCM or ITU-T G.711.  ``wav`` may also hold codes already --
    int16 for 'pcm16', uint8 for the three 8-bit encodings -- which are written as they are."""
    if encoding not in ENCODINGS:
        raise ValueError('save_wav: encoding must be one of {}, got {!r}'.format(', '.join(sorted(ENCODINGS)), encoding))
    tag, dtype = ENCODINGS[encoding]
    wav = np.asarray(wav)
    if wav.dtype.kind in 'iu':
        if encoding == 'float32' or wav.dtype != dtype:
            raise ValueError('save_wav: {} codes cannot be written as {!r} ({} codes are needed)'.format(wav.dtype, encoding, np.dtype(dtype)))
        if norm:
            raise ValueError('save_wav: codes cannot be normalised')
        _write_coded_wav(wav_path, wav, sampling_rate, tag)
        return
    wav = wav.astype(np.float32)
    if norm:
        eng = engine or default_engine()
        flat = wav.reshape(1, -1)            # inf-norm over the whole array (axis=None)
        wav = eng.peak_normalize(eng.to_device(flat)).to_host().reshape(wav.shape)
    if encoding == 'float32':
        _write_float32_wav(wav_path, wav, sampling_rate)
        return
    if wav.ndim not in (1, 2) or wav.size < 1:
        raise ValueError('save_wav: samples (n,) or (channels, n) are needed, got shape {}'.format(wav.shape))
    eng = engine or default_engine()
    codes, _stats = eng.encode(wav, encoding, dither='tpdf' if dither else None, seed=0)
    _write_coded_wav(wav_path, codes, sampling_rate, tag)


def _g711_tables():
    """the 256 values of g711.c's ulaw2linear and alaw2linear, as int16: (mu-law, A-law)"""
    c = np.arange(256, dtype=np.int64)
    u = ~c & 0xFF
    t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
    mulaw = np.where(u & 0x80, 0x84 - t, t - 0x84)
    a = c ^ 0x55
    t, seg = (a & 0xF) << 4, (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    alaw = np.where(a & 0x80, t, -t)
    return mulaw.astype(np.int16), alaw.astype(np.int16)


MULAW_TABLE, ALAW_TABLE = _g711_tables()


def _read_wav(path):
    """-> (format tag, channels, rate, bits, raw data bytes) of a RIFF/WAVE file.  A G.711 file must have the extended fmt chunk
    (18 bytes or more) that the WAVE format asks of every non-PCM format: with the 16 bytes of a PCM header it is refused."""
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
            elif tag in (_ALAW, _MULAW) and len(body) < 18:
                raise ValueError('{}: unsupported WAV format tag {} with {} bits per sample in a {}-byte fmt chunk (G.711 needs the '
                                 'extended chunk)'.format(path, tag, bits, len(body)))
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
    (float32 mono samples, native rate).  PCM 8 (unsigned), 16, 24, 32 bit, IEEE float32 / float64 and 8-bit ITU-T G.711 mu-law /
    A-law (format tags 7 and 6: the codes go through g711.c's decode tables to 16-bit values); integers scaled by
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
    elif tag in (_ALAW, _MULAW) and bits == 8:
        n = len(raw) // channels
        table = MULAW_TABLE if tag == _MULAW else ALAW_TABLE
        x = table[np.frombuffer(raw[:n * channels], dtype=np.uint8)].astype(np.float32) * np.float32(1.0 / 32768.0)
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
