"""GPU: the dataset feature kernels of csrc/features.hip (trim_mse_kernel, trim_bounds_kernel, feat2048_kernel,
feat_generic_kernel) element by element against the float64 oracle, over the table of feature_cases.py -- the bound and
the exact checks are described there, and test_feature_bounds_host.py shows on the same inputs that plain float32
arithmetic keeps a fourfold margin to it.  Also here: the table cache of a handle with one field changed at a time, the
trim decision at other frame lengths and hops and on recordings of more than 256 trim frames (the strided loops of
trim_bounds_kernel), every refusal of the three entry points, and non-finite samples (a NaN is carried, never turned into
-100 dB or dropped from the maximum: "Non-finite values" in include/sstts_hip.h)."""
import ctypes

import numpy as np
import pytest

import audio_cases as AC
import feature_cases as FC
import trim_oracle as T
from conftest import pkg

pytestmark = pytest.mark.gpu
F32 = np.float32
TTS_OK, TTS_ERR_INVALID, TTS_ERR_UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope='module')
def eng():
    e = pkg().Engine()
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1])) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('index', range(len(FC.CASES)))
def test_feature_rows_within_the_interval(eng, index):
    c = FC.CASES[index]
    out = eng.extract_features(list(FC.recordings(index)), eng.feature_params(**FC.param_fields(c)))
    refs = FC.case_oracle(index)
    assert [tuple(p[:2]) for p in eng.last_feature_plan.tolist()] == [(r.start, r.end) for r in refs]
    bad, infos = FC.check_case(index, out)
    print('features {}: worst |implied magnitude - m| / d_t: mel {:.3f} lin {:.3f}'.format(
        c.name, max(i['mel_ratio'] for i in infos), max(i['lin_ratio'] for i in infos)))
    assert not bad, bad


# ----------------------------------------------------------------------------------------------- the table cache
def test_one_handle_one_field_changed_at_a_time(eng):
    """feat_tables keys its window on win_length and its filter bank on n_fft, sampling_rate, n_mels, fmin and fmax: a key
    that misses a field would serve the previous step's table"""
    first = dict(n_fft=2048, win_length=1102, hop_length=275, sampling_rate=22050, n_mels=80, fmin=0.0, fmax=8000.0)
    steps = [dict(), dict(fmin=125.0), dict(sampling_rate=16000, fmax=0.0), dict(n_mels=144), dict(win_length=1103), dict(n_fft=4096)]
    wavs = [AC.broadband(np.random.default_rng(77), 275 * 9 + 3, b) for b in range(2)]
    fields = dict(first)
    seen = []
    for k, change in enumerate(steps + [first]):
        fields.update(change)
        out = eng.extract_features(wavs, eng.feature_params(normalize=k % 2, reduction=2, trim=0, **fields))
        cfg = tuple(fields[f] for f in ('n_fft', 'win_length', 'hop_length', 'sampling_rate', 'n_mels', 'fmin', 'fmax'))
        for b, (w, (mel, lin)) in enumerate(zip(wavs, out)):
            ref = FC.oracle(w, cfg, 2)
            bad, _ = FC.check_rows(mel.reshape(-1, cfg[4]), lin.reshape(-1, 1 + cfg[0] // 2), ref, k % 2, 'step {} {} b{}'.format(k, change, b))
            assert not bad, bad
        seen.append(out)
    assert _same_bits(seen[0], seen[-1])


# ----------------------------------------------------------------------------------------------- trim bounds
TRIM_SHAPES = [(2048, 512), (1024, 256), (400, 100), (256, 64), (256, 300)]
TOP_DBS = (20, 40, 60)


def _trim_lengths(L, H):
    """the shortest legal length, one below / at / one above a multiple of the hop beyond the frame length, an odd one"""
    m = H * (-(-L // H) + 7)
    return [L // 2 + 1, m - 1, m, m + 1, 23 * H + 17]


def _trim_recording(rng, n, k, L, H):
    """speech between quiet margins whose sizes go round with k (none, leading, trailing, both), n samples in all; drawn
    again while a frame's level sits within 1e-3 dB of one of the thresholds"""
    lead = (0, n // 3, 0, n // 4)[k % 4]
    trail = (0, 0, n // 3, n // 5)[k % 4]
    while True:
        w = FC.speechlike(rng, n - lead - trail, lead, trail)
        if min(T.threshold_margin(w, top_db, L, H) for top_db in TOP_DBS) > 1e-3:
            return w


def _assert_trim(eng, wavs, L, H, top_db):
    for w in wavs:
        assert T.threshold_margin(w, top_db, L, H) > 1e-3
    ref = np.array([T.trim_bounds(w, top_db, L, H) for w in wavs])
    got = eng.trim_bounds(wavs, L, H, top_db)
    assert got.dtype == np.int64 and np.array_equal(got, ref), (L, H, top_db, got.tolist(), ref.tolist())
    return ref


@pytest.mark.parametrize('top_db', TOP_DBS)
@pytest.mark.parametrize('L,H', TRIM_SHAPES)
def test_trim_bounds_other_frames_and_hops(eng, L, H, top_db):
    rng = np.random.default_rng(L + H)
    singles = [_trim_recording(rng, n, k, L, H) for k, n in enumerate(_trim_lengths(L, H))]
    for w in singles:
        _assert_trim(eng, [w], L, H, top_db)                       # B = 1
    lengths = _trim_lengths(L, H)
    ragged = [_trim_recording(rng, lengths[k % 5] + (k // 5) * H + k % 3, k, L, H) for k in range(33)]
    ref = _assert_trim(eng, ragged, L, H, top_db)
    assert len({tuple(r) for r in ref.tolist()}) > 10              # (the batch does not ask one question 33 times)


def _smallest(lo, hi, pred):
    """smallest x of lo .. hi with pred(x), for a pred that turns from false to true once"""
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
    return lo


def _long_recording(first, last, top_db, L=256, H=64, n=38400 + 37):
    """Exact zeros, a moderate tone (-10 dB) from an onset to an offset and the loudest stretch in frames 300 .. 400.  A
    frame's energy falls as the onset moves right and grows as the offset does, so each is found by bisection: the
    sample at which the float64 decision moves on by one frame, and from there half a hop into the wanted frame's range."""
    t = np.arange(n)
    tone = 0.3 * np.sin(2 * np.pi * 0.11 * t + 0.3)

    def build(a, b):
        y = np.zeros(n)
        y[a:b] = tone[a:b]
        y[300 * H:400 * H] = np.sin(2 * np.pi * 0.07 * t[300 * H:400 * H])
        return y.astype(np.float32)

    a = _smallest(first * H - L, first * H + L, lambda a: T.trim_bounds(build(a, 450 * H), top_db, L, H)[0] > first * H) - H // 2
    b = _smallest(last * H - L, last * H + L, lambda b: T.trim_bounds(build(a, b), top_db, L, H)[1] >= (last + 1) * H) + H // 2
    return build(a, b)


@pytest.mark.parametrize('top_db', TOP_DBS)
def test_trim_bounds_beyond_256_frames(eng, top_db):
    """601 trim frames against the 256 threads of trim_bounds_kernel: its loops run a second and a third pass, and the
    first frame, the last frame and the maximum each come out of a pass other than the first"""
    L, H = 256, 64
    wavs = [_long_recording(first, last, top_db) for first, last in ((255, 511), (256, 512), (257, 511), (256, 511), (257, 512))]
    for w in wavs:
        mse, _ = T.frame_power_db(w, L, H)
        assert len(mse) == 601 and int(np.argmax(mse)) >= 300 and not mse[:250].any() and not mse[520:].any()
    ref = _assert_trim(eng, wavs, L, H, top_db)
    assert ref.tolist() == [[255 * H, 512 * H], [256 * H, 513 * H], [257 * H, 512 * H], [256 * H, 512 * H], [257 * H, 513 * H]]


# ----------------------------------------------------------------------------------------------- refusals
def _raw_call(eng, wav, p, plan=None, mel_shift=0, extract=True):
    """tts_plan_features (unless a plan is given) and tts_extract_features on one recording -> (status, message)"""
    d = eng.to_device(np.ascontiguousarray(wav, dtype=np.float32))
    offsets = np.array([0, len(wav)], dtype=np.int64)
    try:
        if plan is None:
            plan = np.zeros(3, dtype=np.int64)
            rc = eng.lib.tts_plan_features(eng.handle, d.ptr, offsets.ctypes.data, 1, ctypes.byref(p), plan.ctypes.data)
            if rc != TTS_OK or not extract:
                return rc, (eng.lib.tts_last_error(eng.handle) or b'').decode()
        plan = np.ascontiguousarray(plan, dtype=np.int64)
        rows = max(int(plan[2]), 1)
        mel = eng.empty((rows, max(p.n_mels, 1) + 1))
        lin = eng.empty((rows, 1 + max(p.n_fft, 2) // 2))
        try:
            rc = eng.lib.tts_extract_features(eng.handle, d.ptr, offsets.ctypes.data, 1, ctypes.byref(p), plan.ctypes.data,
                                              mel.data_ptr() + mel_shift, lin.data_ptr())
            eng.synchronize()
            return rc, (eng.lib.tts_last_error(eng.handle) or b'').decode()
        finally:
            mel.free()
            lin.free()
    finally:
        d.free()


def test_refusals_leave_the_handle_usable(eng):
    rng = np.random.default_rng(3)
    w = FC.speechlike(rng, 5000, 3000, 2500)
    good = eng.extract_features([w])
    P = eng.feature_params
    PARAMS = 'features: '
    bad_struct = P()
    bad_struct.struct_size = 4
    spike = np.zeros(6000, np.float32)
    spike[3000] = 1.0                 # trim frames of 1024 at hop 512: frames 5 and 6 hold it, the segment is 2560 .. 3584
    assert T.trim_bounds(spike, 60, 1024, 512) == (2560, 3584)
    refusals = [
        ('struct_size', TTS_ERR_INVALID, PARAMS + 'params missing or not from tts_default_feature_params (struct_size)', dict(p=bad_struct)),
        ('n_fft 384', TTS_ERR_UNSUPPORTED, PARAMS + 'n_fft must be a power of two from 256 to 4096', dict(p=P(n_fft=384, win_length=300))),
        ('n_fft 8192', TTS_ERR_UNSUPPORTED, PARAMS + 'n_fft must be a power of two from 256 to 4096', dict(p=P(n_fft=8192))),
        ('win > n_fft', TTS_ERR_INVALID, PARAMS + 'need 2 <= win_length <= n_fft, hop_length >= 1', dict(p=P(win_length=2049))),
        ('hop 0', TTS_ERR_INVALID, PARAMS + 'need 2 <= win_length <= n_fft, hop_length >= 1', dict(p=P(hop_length=0))),
        ('reduction 0', TTS_ERR_INVALID, PARAMS + 'bad sampling_rate / n_mels / fmin / reduction', dict(p=P(reduction=0))),
        ('n_mels 0', TTS_ERR_INVALID, PARAMS + 'bad sampling_rate / n_mels / fmin / reduction', dict(p=P(n_mels=0))),
        ('n_mels 4097', TTS_ERR_INVALID, PARAMS + 'bad sampling_rate / n_mels / fmin / reduction', dict(p=P(n_mels=4097))),
        ('NaN fmin', TTS_ERR_INVALID, PARAMS + 'bad sampling_rate / n_mels / fmin / reduction', dict(p=P(fmin=float('nan')))),
        ('top_db 0', TTS_ERR_INVALID, PARAMS + 'trim needs frame_length >= 2, hop_length >= 1, top_db > 0', dict(p=P(trim_top_db=0.0))),
        ('n_fft / 2 samples', TTS_ERR_INVALID, 'plan_features: recording 0: the analysed segment has 1024 samples, at most n_fft / 2 '
         '(reflect padding undefined)', dict(p=P(trim=0), wav=w[3000:4024])),
        ('trimmed to n_fft / 2', TTS_ERR_INVALID, 'plan_features: recording 0: the analysed segment has 1024 samples, at most n_fft / 2 '
         '(reflect padding undefined)', dict(p=P(trim_frame_length=1024), wav=spike)),
        ('plan: end beyond', TTS_ERR_INVALID, 'extract_features: plan entry 0 does not match the recording and parameters '
         '(from tts_plan_features)', dict(p=P(trim=0), plan=[0, len(w) + 1, 5 * (-(-(1 + (len(w) + 1) // 275) // 5))])),
        ('plan: wrong T_pad', TTS_ERR_INVALID, 'extract_features: plan entry 0 does not match the recording and parameters '
         '(from tts_plan_features)', dict(p=P(trim=0), plan=[0, len(w), 5 * (-(-(1 + len(w) // 275) // 5)) + 5])),
        ('misaligned output', TTS_ERR_INVALID, 'extract_features: float buffers must be 4-byte aligned', dict(p=P(trim=0), mel_shift=2)),
    ]
    # the plan entries above are right but for the one thing each names
    assert _raw_call(eng, w, P(trim=0), plan=[0, len(w), 5 * (-(-(1 + len(w) // 275) // 5))])[0] == TTS_OK
    for name, status, message, kw in refusals:
        rc, msg = _raw_call(eng, kw.pop('wav', w), **kw)
        assert rc == status and msg == message, (name, rc, msg)
        assert _same_bits(eng.extract_features([w]), good), name


# ----------------------------------------------------------------------------------------------- non-finite samples
NONFINITE_CONFIGS = [(2048, 1102, 275, 8000), (512, 400, 100, 3000)]


def _covered(n_fft, win, hop, p, Tf):
    """frames whose win_length span holds sample p (the zero padding of a window shorter than n_fft does not count)"""
    t = np.arange(Tf)
    lo = t * hop - n_fft // 2 + (n_fft - win) // 2
    return (lo <= p) & (p < lo + win)


def _nonfinite_run(eng, n_fft, win, hop, n, normalize, value):
    rng = np.random.default_rng(n_fft + normalize)
    wavs = [FC.speechlike(rng, n + 13 * b) for b in range(3)]
    p = eng.feature_params(n_fft=n_fft, win_length=win, hop_length=hop, normalize=normalize, reduction=2, trim=0)
    clean = eng.extract_features(wavs, p)
    pos = len(wavs[1]) // 2
    assert pos > n_fft and len(wavs[1]) - pos > n_fft           # (no reflection carries the sample to a second place)
    dirty = [w.copy() for w in wavs]
    dirty[1][pos] = value
    out = eng.extract_features(dirty, p)
    assert _same_bits([out[0], out[2]], [clean[0], clean[2]])    # both neighbours
    Tf = 1 + len(wavs[1]) // hop
    cov = _covered(n_fft, win, hop, pos, Tf)
    assert 2 <= cov.sum() <= win // hop + 1 and not cov[0] and not cov[-1]
    F = 1 + n_fft // 2
    mel, lin = out[1][0].reshape(-1, 80), out[1][1].reshape(-1, F)
    mel0, lin0 = clean[1][0].reshape(-1, 80), clean[1][1].reshape(-1, F)
    keep = np.ones(len(mel), bool)
    keep[:Tf] = ~cov
    assert np.array_equal(_bits(mel[keep]), _bits(mel0[keep])) and np.array_equal(_bits(lin[keep]), _bits(lin0[keep]))
    empty = ~FC.bank_of((n_fft, win, hop, 22050, 80, 0.0, 8000.0)).any(axis=1)
    hit = np.flatnonzero(cov)
    assert np.array_equal(_bits(mel[hit][:, empty]), _bits(mel0[hit][:, empty]))      # an empty band reads no magnitude
    return mel[hit][:, ~empty], lin[hit]


@pytest.mark.parametrize('normalize', [0, 1])
@pytest.mark.parametrize('n_fft,win,hop,n', NONFINITE_CONFIGS)
def test_a_nan_sample_is_nan_in_exactly_the_frames_that_cover_it(eng, n_fft, win, hop, n, normalize):
    mel, lin = _nonfinite_run(eng, n_fft, win, hop, n, normalize, np.nan)
    assert np.isnan(lin).all(), 'a NaN sample became a finite linear value ({} of {})'.format((~np.isnan(lin)).sum(), lin.size)
    assert np.isnan(mel).all(), 'a NaN sample became a finite mel value ({} of {})'.format((~np.isnan(mel)).sum(), mel.size)


@pytest.mark.parametrize('normalize', [0, 1])
@pytest.mark.parametrize('n_fft,win,hop,n', NONFINITE_CONFIGS)
def test_an_inf_sample_is_nan_or_the_image_of_inf(eng, n_fft, win, hop, n, normalize):
    mel, lin = _nonfinite_run(eng, n_fft, win, hop, n, normalize, np.inf)
    image = F32(1.0) if normalize else F32(np.inf)
    assert (np.isnan(lin) | (lin == image)).all() and (np.isnan(mel) | (mel == image)).all()


def test_trim_decides_on_a_non_finite_recording_as_numpy_does(eng):
    """numpy's max carries a NaN, every comparison with it is false, no frame is non-silent: (0, 0), which is also what a
    +-Inf sample gives (Inf - Inf in its frames, -Inf in the others); tts_plan_features then refuses that recording by name"""
    rng = np.random.default_rng(21)
    L, H = 256, 64
    base = [FC.speechlike(rng, 3000, 700, 900), FC.speechlike(rng, 40000, 500, 500), FC.speechlike(rng, 2000, 300, 0)]
    clean = eng.trim_bounds(base, L, H, 40)
    assert np.array_equal(clean, np.array([T.trim_bounds(w, 40, L, H) for w in base]))
    for value in (np.nan, np.inf, -np.inf):
        for b, pos in ((0, 1500), (1, 64 * 300 + 5), (1, 11), (2, 1999)):      # frames of the first pass and of the second
            wavs = [w.copy() for w in base]
            wavs[b][pos] = value
            ref = np.array([T.trim_bounds(w, 40, L, H) for w in wavs])
            assert tuple(ref[b]) == (0, 0)
            got = eng.trim_bounds(wavs, L, H, 40)
            assert np.array_equal(got, ref), (value, b, pos, got.tolist())
    wavs = [w.copy() for w in base]
    wavs[1][20000] = np.nan
    with pytest.raises(pkg().TtsError, match=r'plan_features: recording 1: the analysed segment has 0 samples, at most n_fft / 2'):
        eng.extract_features(wavs)
    assert np.array_equal(eng.trim_bounds(base, L, H, 40), clean)
