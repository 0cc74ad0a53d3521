"""The delivery encoder with no GPU: the numpy oracle (tests/encode_oracle.py) against ITU-T G.711 as the standard library has it
and against the rules of include/sstts_hip.h -- ties, saturation, special values, the dither's moments -- the WAV containers of
audio.io for the four encodings, and what the binding checks and refuses before it touches a handle."""
import wave

import numpy as np
import pytest

import encode_cases as C
import encode_oracle as O
from conftest import pkg
from host_checks import no_device_engine

ALL16 = np.arange(-32768, 32768, dtype=np.int64)


def test_the_oracles_g711_is_audioops_on_every_16_bit_value():
    audioop = pytest.importorskip('audioop')
    raw = ALL16.astype('<i2').tobytes()
    assert np.array_equal(O.lin2ulaw(ALL16), np.frombuffer(audioop.lin2ulaw(raw, 2), np.uint8))
    assert np.array_equal(O.lin2alaw(ALL16), np.frombuffer(audioop.lin2alaw(raw, 2), np.uint8))
    codes = bytes(range(256))
    assert np.array_equal(O.ULAW_TABLE, np.frombuffer(audioop.ulaw2lin(codes, 2), '<i2'))
    assert np.array_equal(O.ALAW_TABLE, np.frombuffer(audioop.alaw2lin(codes, 2), '<i2'))


def test_every_g711_code_survives_its_decode_table():
    """encode(decode(c)) == c for every code but mu-law 0x7F, the negative zero, which decodes to 0 and encodes as 0xFF"""
    c = np.arange(256)
    back = O.lin2ulaw(O.ULAW_TABLE)
    assert np.array_equal(np.flatnonzero(back != c), [0x7F]) and back[0x7F] == 0xFF and O.ULAW_TABLE[0x7F] == 0
    assert np.array_equal(O.lin2alaw(O.ALAW_TABLE), c)
    assert O.lin2ulaw(0) == 0xFF == O.SILENCE[O.MULAW] and O.lin2alaw(0) == 0xD5 == O.SILENCE[O.ALAW]
    # monotone: a larger 16-bit value never decodes to a smaller one
    for enc, table in ((O.lin2ulaw, O.ULAW_TABLE), (O.lin2alaw, O.ALAW_TABLE)):
        assert np.all(np.diff(table[enc(ALL16)].astype(np.int64)) >= 0)
    # the product's tables (audio.io) are the oracle's
    io = pkg('audio.io')
    assert np.array_equal(io.MULAW_TABLE, O.ULAW_TABLE) and np.array_equal(io.ALAW_TABLE, O.ALAW_TABLE)


def test_every_level_encodes_to_itself():
    x = C.all_levels()
    codes, st = O.encode(x[None], O.S16)
    assert np.array_equal(codes[0], ALL16) and tuple(st[0]) == (0, 0, 32768, 65536)
    assert np.array_equal(O.encode(x[None], O.MULAW)[0][0], O.lin2ulaw(ALL16))
    assert np.array_equal(O.encode(x[None], O.ALAW)[0][0], O.lin2alaw(ALL16))
    # pcm8: 256 float32 samples to every 8-bit level; k / 128 + 1 / 256 is a tie between two levels and goes to the even one
    codes8 = O.encode(x[None], O.U8)[0][0].astype(np.int64)
    k = np.arange(-128, 128)
    assert np.array_equal(codes8[::256], k + 128)
    ties = codes8[128::256] - 128
    assert np.all(ties[:-1] % 2 == 0) and np.all(np.abs(ties[:-1] - (k[:-1] + 0.5)) == 0.5) and ties[-1] == 127   # (127.5 -> 128: saturated)


def test_ties_go_to_the_even_integer():
    for k, want in ((0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (-2.5, -2)):
        x = np.array([[k * C.LSB]], np.float32)
        assert O.encode(x, O.S16)[0][0, 0] == want, k
        assert O.encode(np.array([[k / 128.0]], np.float32), O.U8)[0][0, 0] == want + 128, k


def test_saturation_and_special_values():
    assert tuple(O.encode(np.array([[1.0]], np.float32), O.S16)[1][0]) == (1, 0, 32767, 1)
    assert O.encode(np.array([[1.0]], np.float32), O.S16)[0][0, 0] == 32767
    assert tuple(O.encode(np.array([[-1.0]], np.float32), O.S16)[1][0]) == (0, 0, 32768, 1)
    assert O.encode(np.array([[-1.0]], np.float32), O.S16)[0][0, 0] == -32768
    x, q, clipped, nans, peak = C.specials()
    codes, st = O.encode(x[None], O.S16)
    assert np.array_equal(codes[0], q) and tuple(st[0]) == (clipped, nans, peak, len(x))
    for fmt, enc in ((O.MULAW, O.lin2ulaw), (O.ALAW, O.lin2alaw)):
        codes, st = O.encode(x[None], fmt)
        assert np.array_equal(codes[0], enc(q)) and tuple(st[0]) == (clipped, nans, peak, len(x))
    codes, st = O.encode(np.array([[1.0, -1.0, np.nan, np.inf, -np.inf, -0.0, 1e-45, 127.5 / 128, -128.5 / 128]], np.float32), O.U8)
    assert codes[0].tolist() == [255, 0, 128, 255, 0, 128, 128, 255, 0] and tuple(st[0]) == (4, 1, 128, 9)


def test_padding_is_silence_and_counts_nowhere():
    x = np.full((3, 9), np.nan, np.float32)
    x[1, 0], x[2] = 2.0, 0.25
    for fmt in O.FORMATS:
        codes, st = O.encode(x, fmt, O.TPDF, 7, n_samples=[0, 1, 9])
        assert np.all(codes[0] == O.SILENCE[fmt]) and np.all(codes[1, 1:] == O.SILENCE[fmt])
        assert tuple(st[0]) == (0, 0, 0, 0) and tuple(st[1])[:2] == (1, 0) and st[1]['n'] == 1 and st[2]['n'] == 9


def test_the_dithers_moments():
    """2^20 samples at seed 1234, row 0.  A triangular d on (-1, 1) has mean 0, variance 1 / 6 and fourth moment 1 / 15: the
    mean's standard error is sqrt(1 / 6 / 2^20) = 4.0e-4 and the variance's sqrt((1 / 15 - 1 / 36) / 2^20) = 1.9e-4, so both
    bounds of 2e-3 are 5 standard errors and more."""
    n = 1 << 20
    d = O.dither(1234, 0, np.arange(n))
    assert abs(d.mean()) < 2e-3, d.mean()
    assert abs(d.var() - 1.0 / 6.0) < 2e-3, d.var()
    assert np.abs(d).max() < 1.0
    # a function of (seed, b, i) alone
    assert np.array_equal(O.dither(1234, 0, np.arange(100, 200)), d[100:200])
    assert not np.array_equal(O.dither(1234, 1, np.arange(100)), d[:100]) and not np.array_equal(O.dither(1235, 0, np.arange(100)), d[:100])
    assert np.array_equal(O.dither(2 ** 63 + 5, 3, np.arange(8)), O.dither(2 ** 63 + 5 + 2 ** 64, 3, np.arange(8)))
    # a constant a quarter of an LSB: the dithered codes average it, the undithered ones lose it
    x = np.full((1, n), 0.25 * C.LSB, np.float32)
    codes = O.encode(x, O.S16, O.TPDF, 1234)[0]
    assert abs(codes.mean() - 0.25) < 2.5e-3, codes.mean()
    assert not O.encode(x, O.S16)[0].any()


@pytest.mark.parametrize('encoding, fmt', [('pcm16', O.S16), ('pcm8', O.U8)])
@pytest.mark.parametrize('channels', [1, 2])
def test_pcm_files_read_back_through_the_standard_library(tmp_path, encoding, fmt, channels):
    io = pkg('audio.io')
    x = np.stack([C.speech_like(301, seed=c) for c in range(channels)])   # (an odd number of bytes for pcm8 mono: the pad byte)
    codes = O.encode(x, fmt, O.TPDF, 0)[0]
    p = str(tmp_path / 'a.wav')
    io.save_wav(p, codes if channels == 2 else codes[0], 8000, encoding=encoding)
    with wave.open(p, 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()) == (channels, O.WIDTH[fmt], 8000, 301, 'NONE')
        raw = w.readframes(301)
    assert np.array_equal(np.frombuffer(raw, '<i2' if fmt == O.S16 else np.uint8).reshape(301, channels).T, codes)


@pytest.mark.parametrize('encoding, fmt', [('pcm16', O.S16), ('pcm8', O.U8), ('mulaw', O.MULAW), ('alaw', O.ALAW)])
def test_every_encoding_round_trips_through_load_wav(tmp_path, encoding, fmt):
    io = pkg('audio.io')
    codes = np.arange(256).astype(O.DTYPE[fmt]) if fmt != O.S16 else ALL16[::37].astype(np.int16)
    p = str(tmp_path / (encoding + '.wav'))
    io.save_wav(p, codes, 8000, encoding=encoding)
    y, sr = io.load_wav(p)
    assert sr == 8000 and y.dtype == np.float32 and np.array_equal(y, O.decode(fmt, codes).astype(np.float32))
    blob = open(p, 'rb').read()
    tag, fmt_size = int.from_bytes(blob[20:22], 'little'), int.from_bytes(blob[16:20], 'little')
    assert (tag, fmt_size, b'fact' in blob[:64]) == {O.S16: (1, 16, False), O.U8: (1, 16, False), O.MULAW: (7, 18, True), O.ALAW: (6, 18, True)}[fmt]
    assert int.from_bytes(blob[4:8], 'little') == len(blob) - 8 and len(blob) % 2 == 0
    # two channels are averaged, as for every other format
    io.save_wav(p, np.stack([codes, codes[::-1]]), 8000, encoding=encoding)
    v = O.decode(fmt, codes).astype(np.float32)
    assert np.array_equal(io.load_wav(p)[0], np.mean(np.stack([v, v[::-1]], axis=1), axis=1, dtype=np.float32))


def test_save_wav_refusals(tmp_path):
    io = pkg('audio.io')
    p = str(tmp_path / 'r.wav')
    with pytest.raises(ValueError, match='encoding'):
        io.save_wav(p, np.zeros(4, np.float32), 8000, encoding='pcm24')
    with pytest.raises(ValueError, match='int16'):
        io.save_wav(p, np.zeros(4, np.int16), 8000, encoding='mulaw')
    with pytest.raises(ValueError, match='float32'):
        io.save_wav(p, np.zeros(4, np.int16), 8000)
    with pytest.raises(ValueError, match='normalised'):
        io.save_wav(p, np.zeros(4, np.uint8), 8000, True, encoding='alaw')


def test_the_output_setting_is_checked_before_a_handle_is_touched():
    H = pkg('_hip')
    S = H.output_setting
    assert S(None) is None
    assert S('pcm16') == (H.FMT_PCM_S16, H.DITHER_TPDF, 0, 0) and S('float32') == H.OUTPUT_OFF == S(('float32', 'tpdf', 8000, 8000))
    assert S(('mulaw', None, 22050, 8000)) == (H.FMT_MULAW, H.DITHER_NONE, 22050, 8000)
    assert S((H.FMT_ALAW, 'tpdf', 22050, 22050)) == (H.FMT_ALAW, H.DITHER_TPDF, 22050, 22050)
    assert H.output_is_on(S('pcm8')) and not H.output_is_on(S('float32')) and not H.output_is_on(S(('float32', None, 8000, 8000)))
    assert H.output_is_on(S(('float32', None, 22050, 11025))) and H.output_ratio(S(('float32', None, 22050, 11025))) == 0.5
    for bad in ('pcm24', 9, True, ('pcm16',), ('pcm16', 'rectangular', None, None), ('pcm16', None, 22050, None), ('pcm16', None, 22050, 0),
                ('pcm16', None, 22050.0, 8000), ('pcm16', None, 22050, 5000), ('pcm16', None, 8000, 32001), ('wav', None, 8000, 8000)):
        with pytest.raises(ValueError):
            S(bad)
    keys = [r.keyword for r in H.SETTINGS]
    row = H.SETTINGS[keys.index('output')]
    assert (row.mirror, row.initial, row.host_only) == ('_output', H.OUTPUT_OFF, True) and row.check is H.output_setting
    assert keys[keys.index('output') - 1:keys.index('output') + 2] == ['limiter', 'output', 'token_times']
    assert [r.keyword for r in H.SETTINGS if r.host_only] == ['output']
    assert [H.FORMATS[k] for k in ('float32', 'pcm16', 'pcm8', 'mulaw', 'alaw')] == [O.F32, O.S16, O.U8, O.MULAW, O.ALAW]
    assert H.ENCODE_RECORD == O.RECORD


def test_the_binding_refuses_before_it_reaches_the_library():
    eng = no_device_engine()
    ids = np.ones((2, 5), np.int32)
    with pytest.raises(ValueError, match=r'Engine\.encode'):
        eng.synthesize(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, output='pcm16')
    with pytest.raises(TypeError):
        eng.synthesize(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, outputs='pcm16')
    for output in ('pcm24', ('pcm16', None, 22050, 5000)):
        with pytest.raises(ValueError):
            eng.synthesize_host(ids, 2, 6.02, 99.89, 1.3, 2, 1102, 275, output=output)
        with pytest.raises(ValueError):
            eng.set_output(output)
    x = np.zeros((2, 8), np.float32)
    for kw in (dict(format='float32'), dict(format='pcm24'), dict(format='pcm16', dither='noise'), dict(format='pcm16', seed=-1),
               dict(format='pcm16', seed=2 ** 64), dict(format='pcm16', n_samples=[1, 9]), dict(format='pcm16', n_samples=[-1, 2]),
               dict(format='pcm16', n_samples=[1]), dict(format='pcm16', n_samples=[1.0, 2.0])):
        with pytest.raises(ValueError):
            eng.encode(x, **kw)
    assert eng._output == pkg('_hip').OUTPUT_OFF


def test_the_library_answers_its_host_only_calls():
    H = pkg('_hip')
    lib = H.load_library()
    assert [lib.tts_encode_width(f) for f in range(5)] == [4, 2, 1, 1, 1] and lib.tts_encode_width(5) < 0 and lib.tts_encode_width(-1) < 0
    assert lib.tts_encode_tile() == H.ENCODE_TILE
    # a NULL handle is refused by every entry point that takes one
    assert lib.tts_set_output(None, 1, 1, 0, 0) == H.TTS_ERR_INVALID
    assert lib.tts_encode(None, None, 1, 1, None, 1, 0, 0, None, None) == H.TTS_ERR_INVALID
