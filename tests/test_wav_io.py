"""audio.io.load_wav (reference audio/io.py:8-30, librosa.core.load at the native rate) on RIFF/WAVE files written here with
`wave` / `struct`: every sample format, mono and stereo, offset / duration, the save_wav round trip, and the refusals."""
import struct
import wave

import numpy as np
import pytest

from conftest import pkg


def io():
    return pkg('audio.io')


def _write_pcm(path, ints, width, sr=16000, channels=1):
    """ints: (n, channels) integer sample codes as stored (8-bit unsigned)."""
    ints = np.asarray(ints).reshape(-1, channels)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        if width == 3:
            v = ints.astype(np.int64).reshape(-1) & 0xFFFFFF
            raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
        else:
            raw = ints.astype({1: np.uint8, 2: '<i2', 4: '<i4'}[width]).tobytes()
        w.writeframes(raw)


def _write_float(path, x, bits, sr=16000, channels=1):
    x = np.asarray(x).reshape(-1, channels).astype('<f%d' % (bits // 8))
    fmt = struct.pack('<HHIIHH', 3, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits)
    data = x.tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 4 + 8 + len(fmt) + 8 + len(data)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<I', len(fmt)) + fmt)
        f.write(b'data' + struct.pack('<I', len(data)) + data)


@pytest.mark.parametrize('bits', [8, 16, 24, 32])
@pytest.mark.parametrize('channels', [1, 2])
def test_pcm_exact_values(tmp_path, bits, channels):
    rng = np.random.default_rng(bits + channels)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    codes = rng.integers(lo, hi + 1, (200, channels))
    codes[0, 0], codes[1, 0] = lo, hi
    stored = codes + 128 if bits == 8 else codes
    p = tmp_path / 'a.wav'
    _write_pcm(p, stored, bits // 8, sr=22050, channels=channels)
    y, sr = io().load_wav(str(p))
    assert sr == 22050 and y.dtype == np.float32 and y.shape == (200,)
    x = codes.astype(np.float32) * np.float32(1.0 / (1 << (bits - 1)))
    ref = x[:, 0] if channels == 1 else np.mean(x, axis=1, dtype=np.float32)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize('bits', [32, 64])
@pytest.mark.parametrize('channels', [1, 2])
def test_float_exact_values(tmp_path, bits, channels):
    x = np.random.default_rng(bits).standard_normal((300, channels)) * 0.3
    p = tmp_path / 'f.wav'
    _write_float(p, x, bits, sr=8000, channels=channels)
    y, sr = io().load_wav(str(p))
    x32 = x.astype('<f%d' % (bits // 8)).astype(np.float32)
    ref = x32[:, 0] if channels == 1 else np.mean(x32, axis=1, dtype=np.float32)
    assert sr == 8000 and np.array_equal(y, ref)


def test_offset_and_duration_rounding(tmp_path):
    codes = np.arange(-500, 500)
    p = tmp_path / 'o.wav'
    _write_pcm(p, codes, 2, sr=1000)
    full, _ = io().load_wav(str(p))
    y, _ = io().load_wav(str(p), offset=0.0125, duration=0.1004)       # 12.5 -> 12 (round half to even), 100.4 -> 100
    assert np.array_equal(y, full[12:112])
    y, _ = io().load_wav(str(p), offset=0.0135)                         # 13.5 -> 14
    assert np.array_equal(y, full[14:])
    y, _ = io().load_wav(str(p), sampling_rate=1000, duration=0.5)
    assert np.array_equal(y, full[:500])


def test_save_load_round_trip_bit_for_bit(tmp_path):
    x = (np.random.default_rng(3).standard_normal(1234) * 0.2).astype(np.float32)
    p = tmp_path / 'r.wav'
    io().save_wav(str(p), x, 22050)
    y, sr = io().load_wav(str(p))
    assert sr == 22050 and np.array_equal(y, x)


def test_resampling_is_refused(tmp_path):
    p = tmp_path / 's.wav'
    _write_pcm(p, np.zeros(10, int), 2, sr=16000)
    with pytest.raises(NotImplementedError, match='resampling'):
        io().load_wav(str(p), sampling_rate=22050)


def test_malformed_files_are_refused(tmp_path):
    p = tmp_path / 'bad.wav'
    p.write_bytes(b'RIFX\x00\x00\x00\x00WAVE')
    with pytest.raises(ValueError, match='bad.wav'):
        io().load_wav(str(p))
    q = tmp_path / 'alaw.wav'
    fmt = struct.pack('<HHIIHH', 6, 1, 8000, 8000, 1, 8)    # A-law: not a format the reader understands
    q.write_bytes(b'RIFF' + struct.pack('<I', 4 + 8 + 16 + 8 + 4) + b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt +
                  b'data' + struct.pack('<I', 4) + b'\x00' * 4)
    with pytest.raises(ValueError, match=r'alaw\.wav.*format tag 6'):
        io().load_wav(str(q))
