"""GPU: the elementwise and reduction kernels of the audio surface at the shapes where they can go wrong --
tts_db_convert past its grid cap (4096 workgroups of 256) and with a ragged tail, in place and out of place, at the
clip edges and the -100 dB limit; tts_denorm_power over frame / bin counts on both sides of its tiles, per utterance;
tts_peak_normalize with the peak at either end of a row, negative, denormal, and a silent row in the batch.

Bounds, element by element against the float64 oracle: mode 0 (magnitude -> dB) claims exact rounding and is held to
equality; modes 2 and 3 to 2 float32 ulps; mode 1 and the de-normalisation to the existing 2e-5 relative; the peak
normalisation to the bits of the oracle.
"""
import numpy as np
import pytest

from oracle import audio_oracle as A

pytestmark = pytest.mark.gpu

REF_DB, MAX_DB = np.float32(6.02), np.float32(99.89)      # as the C entry points receive them: floats
DB_SIZES = [1, 255, 257, 4096 * 256 + 1, 3 * 4096 * 256 + 77]
TTS_OK, TTS_ERR_DB_RANGE = 0, -4
F32 = np.float32


def _convert(engine, x, mode, in_place):
    """-> (status, output, the input buffer afterwards)"""
    d_in = engine.to_device(x)
    d_out = d_in if in_place else engine.to_device(np.full(x.shape, 777.0, np.float32))
    rc = engine.lib.tts_db_convert(engine.handle, d_in.ptr, x.size, mode, float(REF_DB), float(MAX_DB), d_out.ptr)
    return rc, d_out.to_host(), d_in.to_host()


def _fill(n, specials, draw, seed):
    """n values: the special ones first (as many as fit), the last of them again at the very end of the ragged tail, random
    ones between"""
    x = draw(np.random.default_rng(seed), n).astype(np.float32)
    k = min(n, len(specials))
    x[:k] = np.asarray(specials, np.float32)[:k]
    if n > len(specials):
        x[-1] = specials[-1]
    return x


def _ulps(got, ref64, scale64):
    """|got - ref| in float32 ulps AT THE SCALE OF THE EXPRESSION'S LARGEST TERM: 1 + q and (c - 1) r + ref cancel near the
    clip edge / near 0 dB, where an ulp of the (tiny) result says nothing about float32 arithmetic on terms of size 1 or
    100 -- numpy's own float32 evaluation is thousands of result-ulps off there."""
    return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.maximum(np.abs(ref64), scale64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('in_place', [True, False])
@pytest.mark.parametrize('n', DB_SIZES)
def test_db_convert_magnitude_to_decibel_is_exactly_rounded(engine, n, in_place):
    tiny = F32(1e-5)
    specials = [0.0, -0.0, -1.5, 1e-40, -1e-40, tiny, np.nextafter(tiny, F32(0)), np.nextafter(tiny, F32(1)), 1.0, 3e38,
                1.17549435e-38, 0.5]
    x = _fill(n, specials, lambda r, k: r.random(k) ** 6 * 30, n)
    rc, y, x_after = _convert(engine, x, 0, in_place)
    assert rc == TTS_OK
    ref = np.float32(20 * np.log10(np.maximum(1e-5, x.astype(np.float64))))
    bad = np.flatnonzero(y != ref)
    assert bad.size == 0, (n, bad[:5], x[bad[:5]], y[bad[:5]], ref[bad[:5]])
    if not in_place:
        assert np.array_equal(x_after.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize('in_place', [True, False])
@pytest.mark.parametrize('n', DB_SIZES)
def test_db_convert_decibel_to_magnitude(engine, n, in_place):
    specials = [-100.0, np.nextafter(F32(-100), F32(0)), 0.0, -0.0, 20.0, -99.99, 6.02, -50.0]   # -100 dB itself is legal
    x = _fill(n, specials, lambda r, k: r.random(k) * 120 - 100, n + 1)
    rc, y, x_after = _convert(engine, x, 1, in_place)
    assert rc == TTS_OK
    ref = np.power(10.0, x.astype(np.float64) / 20.0)
    rel = np.abs(y - ref) / ref
    print('dB -> magnitude n={}: worst relative error {:.3e}'.format(n, rel.max()))
    assert rel.max() <= 2e-5
    if not in_place:
        assert np.array_equal(x_after.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize('n', DB_SIZES)
def test_db_convert_refuses_below_minus_100_db_and_rearms(engine, n):
    """the first float below -100 dB, at the END of the ragged tail, refuses the call; the legal call straight after it
    succeeds (the device flag is armed per call) and gives the right numbers"""
    x = _fill(n, [-100.0], lambda r, k: r.random(k) * 120 - 100, n + 2)
    bad = x.copy()
    bad[-1] = np.nextafter(F32(-100), F32(-np.inf))
    rc, _, _ = _convert(engine, bad, 1, True)
    assert rc == TTS_ERR_DB_RANGE
    assert b'-100 dB' in engine.lib.tts_last_error(engine.handle)
    rc, y, _ = _convert(engine, x, 1, True)
    assert rc == TTS_OK
    ref = np.power(10.0, x.astype(np.float64) / 20.0)
    assert (np.abs(y - ref) / ref).max() <= 2e-5


@pytest.mark.parametrize('in_place', [True, False])
@pytest.mark.parametrize('n', DB_SIZES)
def test_db_convert_normalize_within_two_ulps(engine, n, in_place):
    r64 = abs(float(REF_DB)) + abs(float(MAX_DB))
    lo, hi = float(REF_DB) - r64, float(REF_DB)          # the dB values that normalise to exactly 0 and 1
    specials = [lo, np.nextafter(F32(lo), F32(0)), np.nextafter(F32(lo), F32(-200)), hi, np.nextafter(F32(hi), F32(0)),
                np.nextafter(F32(hi), F32(100)), -150.0, 50.0, -1e30, 1e30, np.inf, -np.inf, 0.0]
    x = _fill(n, specials, lambda r, k: r.random(k) * 200 - 150, n + 3)     # both clip sides
    rc, y, x_after = _convert(engine, x, 2, in_place)
    assert rc == TTS_OK
    with np.errstate(invalid='ignore'):
        q = (x.astype(np.float64) - float(REF_DB)) / r64
        ref = A.normalize_decibel(x.astype(np.float64), float(REF_DB), float(MAX_DB))
    assert (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1)).any() or n < 3
    u = _ulps(y, ref, np.minimum(np.maximum(np.abs(q), 1.0), 2.0))
    print('normalize n={}: worst {:.2f} ulp'.format(n, u.max()))
    assert u.max() <= 2.0
    assert y.min() >= 0.0 and y.max() <= 1.0
    if not in_place:
        assert np.array_equal(x_after.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize('in_place', [True, False])
@pytest.mark.parametrize('n', DB_SIZES)
def test_db_convert_inv_normalize_within_two_ulps(engine, n, in_place):
    specials = [0.0, -0.0, 1.0, np.nextafter(F32(0), F32(1)), np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)),
                -0.2, 1.2, -1e30, 1e30, np.inf, -np.inf, 1e-40, 0.5]
    x = _fill(n, specials, lambda r, k: r.random(k) * 1.4 - 0.2, n + 4)       # both clip sides
    rc, y, x_after = _convert(engine, x, 3, in_place)
    assert rc == TTS_OK
    r64 = abs(float(REF_DB)) + abs(float(MAX_DB))
    ref = A.inv_normalize_decibel(x.astype(np.float64), float(REF_DB), float(MAX_DB))
    u = _ulps(y, ref, np.full(ref.shape, r64))
    print('inv_normalize n={}: worst {:.2f} ulp'.format(n, u.max()))
    assert u.max() <= 2.0
    assert y.min() >= float(REF_DB) - r64 - 1e-5 and y.max() <= float(REF_DB)
    if not in_place:
        assert np.array_equal(x_after.view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------------------------ tts_denorm_power
DENORM_SHAPES = [(1, 1, 1025), (3, 31, 1025), (2, 33, 513), (1, 1000, 1025), (2, 40, 129)]


@pytest.mark.parametrize('power', [1.0, 1.3, 2.0])
@pytest.mark.parametrize('B,T,F', DENORM_SHAPES)
def test_denorm_power_shapes(engine, B, T, F, power):
    rng = np.random.default_rng(B * 10000 + T * 10 + F)
    lin = (rng.random((B, T, F)) * 1.4 - 0.2).astype(np.float32)       # both clip sides
    lin[0, 0, 0], lin[-1, -1, -1] = 0.0, 1.0                           # the floor and the ceiling at the two corners
    mag = engine.denorm_power(lin, float(REF_DB), float(MAX_DB), power).to_host()
    assert mag.shape == (B, F, T)
    for b in range(B):
        ref = A.linear_to_magnitude(lin[b].astype(np.float64), float(REF_DB), float(MAX_DB), power)
        assert ref.shape == (F, T)
        # utterance b's frames, transposed, and nobody else's: each utterance has its own random numbers
        assert np.allclose(mag[b], ref, rtol=2e-5, atol=0), (b, np.abs(mag[b] / ref - 1).max())
    lo = 10.0 ** ((float(REF_DB) - abs(float(REF_DB)) - abs(float(MAX_DB))) / 20.0 * power)
    assert abs(mag[0, 0, 0] / lo - 1) <= 2e-5 and abs(mag[-1, -1, -1] / 10.0 ** (float(REF_DB) / 20.0 * power) - 1) <= 2e-5


@pytest.mark.parametrize('B,T,F', DENORM_SHAPES)
def test_denorm_power_range_check_sees_the_last_row_of_the_last_utterance(engine, B, T, F):
    """constants that allow a value below -100 dB (ref -50, max 99.89: the floor is -199.89 dB): the one offending value
    sits in the last frame of the last utterance; without it the same call succeeds (the flag is armed per call)"""
    lin = np.full((B, T, F), 0.9, np.float32)                           # -64.989 dB
    bad = lin.copy()
    bad[-1, -1, F // 2] = 0.6                                            # -109.956 dB
    with pytest.raises(AssertionError):
        engine.denorm_power(bad, -50.0, 99.89, 1.3)
    mag = engine.denorm_power(lin, -50.0, 99.89, 1.3).to_host()
    ref = A.linear_to_magnitude(lin[0].astype(np.float64), -50.0, 99.89, 1.3)
    assert np.allclose(mag[0], ref, rtol=2e-5, atol=0)


# ------------------------------------------------------------------------------------------------ tts_peak_normalize
@pytest.mark.parametrize('n', [1, 63, 1025, 275 * 999])
@pytest.mark.parametrize('where', ['first', 'last', 'negative'])
def test_peak_normalize_peak_positions(engine, n, where):
    rng = np.random.default_rng(n)
    wav = (rng.standard_normal((5, n)) * 0.01).astype(np.float32)
    wav[3] = 0.0                                                         # one silent row: left alone
    wav[4] = (rng.standard_normal(n) * 1e-41).astype(np.float32)         # a row whose peak is denormal: left alone
    i = {'first': 0, 'last': n - 1, 'negative': n // 2}[where]
    for b in range(3):
        wav[b, i] = -0.75 - b if where == 'negative' else 0.5 + b
    got = engine.peak_normalize(engine.to_device(wav)).to_host()
    for b in range(5):
        assert np.array_equal(got[b].view(np.uint32), A.peak_normalize(wav[b]).view(np.uint32)), (n, where, b)
    assert np.array_equal(got[3:].view(np.uint32), wav[3:].view(np.uint32))
    assert np.all(np.abs(got[:3]).max(axis=1) == 1.0)
