"""Cases, signals, the element-by-element bound and a float32 restatement for the dataset feature kernels of
csrc/features.hip (a plain helper module, imported like audio_cases.py and trim_oracle.py).

test_gpu_feature_bounds.py runs every case of CASES through Engine.extract_features and test_feature_bounds_host.py runs the
float32 restatement below (and a set of deliberately wrong float64 ones) over the SAME inputs, both under check_rows().

The bound.  Let m be the float64 oracle's magnitude of one frame -- |STFT| for the linear row, bank @ |STFT| for the mel
row -- and d_t = ANALYSIS_TOL max(m[t, :]) over the frame's own row (the 1e-5 of the analysis side, audio_cases.py).  A
value must lie in [f(max(m - d_t, 0)), f(m + d_t)] with f = magnitude_to_decibel in float64, widened by one float32 ulp of
the dB value, and, when normalised, normalize_decibel of that with the constants as the floats the C entry point receives,
widened by two float32 ulps at the scale of the expression's largest term (the _ulps scale of test_gpu_elementwise.py) and
cut to [0, 1].  The form is right at the 1e-5 floor and at the clips, where a linearised dB tolerance is not: a frame of
exact zeros has d_t = 0 and demands the floor value.  On top of the interval, bit for bit: all-zero frames and empty mel
bands are the float32 image of -100 dB, reduction padding rows are 0, the DC bin of a full-scale constant, normalised,
is 1.0.
"""
import collections
import functools

import numpy as np

import audio_cases as AC
import trim_oracle as T
from oracle import audio_oracle as A

ANALYSIS_TOL = AC.ANALYSIS_TOL
HOST_MARGIN = AC.HOST_MARGIN
INFORMATIVE_DB = 0.05            # an element whose interval half-width exceeds this is near the floor: the bound says little
CONSTS = (6.02, 99.89, 35.66, 100.0)     # mel_ref_db, mel_max_db, linear_ref_db, linear_max_db (LJSpeechDatasetHelper)
SR = 22050
F32 = np.float32


# ----------------------------------------------------------------------------------------------- signals
def speechlike(rng, n, lead=0, trail=0, floor_db=-40.0, quiet=1e-5):
    """Tones with a syllable envelope plus a noise floor `floor_db` below the peak, between margins of quiet noise.  A small DC
    offset and a small component at the Nyquist frequency keep the two real-valued bins off the 1e-5 magnitude floor: under
    noise alone they are Gaussian, not Rayleigh, and come near zero in about one frame in a thousand, where the float32
    transform's absolute error (~4e-7 here) is a large part of a dB value."""
    t = np.arange(n) / SR
    f0 = rng.uniform(90, 220)
    x = np.zeros(n)
    for h in range(1, 12):
        x += rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * f0 * h * t * (1 + 0.02 * np.sin(2 * np.pi * 3 * t)) + rng.uniform(0, 6.3))
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2, 5) * t + rng.uniform(0, 6.3))
    x *= 0.5 / np.max(np.abs(x))
    x += 0.5 * 10 ** (floor_db / 20) * rng.standard_normal(n)
    x += 2e-3 * (1.0 + (-1.0) ** np.arange(n))
    out = quiet * rng.standard_normal(lead + n + trail)
    out[lead:lead + n] = x
    return out.astype(np.float32)


def gapped(rng, n, n_fft):
    """speech-like with an interior stretch of exact zeros 3 n_fft + 1 samples long (so some frames are entirely zero) and
    the last quarter scaled by 1e-4 (so some frames lie near the 1e-5 floor)"""
    gap = 3 * n_fft + 1
    assert n >= gap + n_fft, (n, n_fft)
    y = speechlike(rng, n).astype(np.float64)
    y[n - n // 4:] *= 1e-4
    g0 = (n - gap) // 3
    y[g0:g0 + gap] = 0.0
    return y.astype(np.float32)


def constant(n):
    """full scale: the DC bin (win / 2) clips to exactly 1.0 when normalised"""
    return np.ones(n, np.float32)


# ----------------------------------------------------------------------------------------------- the table
# (n_fft, win, hop, sr, n_mels, fmin, fmax); fmax <= 0: sr / 2.  The first three run feat2048_kernel, the others
# feat_generic_kernel; 144 channels are more than two passes of the 2048 kernel's 64 lanes; 128 channels over 257 bins
# leave empty bands; the last two are a hop of 1 and a hop above n_fft.
CONFIGS = [(2048, 1102, 275, 22050, 80, 0.0, 8000.0),
           (2048, 2048, 512, 22050, 80, 0.0, 8000.0),
           (2048, 1103, 275, 22050, 144, 125.0, 7600.0),
           (256, 200, 50, 16000, 40, 50.0, 7600.0),
           (512, 400, 100, 22050, 128, 0.0, 0.0),
           (1024, 1024, 256, 22050, 80, 0.0, -1.0),
           (4096, 2400, 600, 22050, 1, 0.0, 8000.0),
           (256, 200, 1, 16000, 40, 50.0, 7600.0),
           (256, 256, 300, 16000, 40, 50.0, 7600.0)]
HOP1_CONFIG, WIDE_HOP_CONFIG, EMPTY_BAND_CONFIG = 7, 8, 4
REDUCTIONS = (1, 2, 5, 7)
BATCHES = (1, 3, 9)
# The signal of a case, by configuration and length index: each kernel meets each signal; `gapped` sits at the longest
# length, where its gap fits.  The full-scale constant goes where the filter bank reaches the main lobe of its DC line.
# Configurations 2 (fmin 125) and 6 (one channel that peaks near 2.8 kHz) see only that line's side lobes: the mel row's
# own maximum lies 50 dB and more below the frame's, d_t of the mel row falls below the float32 transform's own rounding
# (about 1e-7 of the DC line per bin), and the float32 restatement itself comes to 1 and 5 d_t there -- the bound says
# nothing about a kernel on such a row, so those two take another signal.
KINDS = (('broadband', 'speechlike', 'constant', 'gapped'),
         ('constant', 'broadband', 'speechlike', 'broadband'),
         ('speechlike', 'broadband', 'broadband', 'gapped'),
         ('broadband', 'speechlike', 'constant', 'gapped'),
         ('constant', 'broadband', 'speechlike', 'broadband'),
         ('speechlike', 'constant', 'broadband', 'gapped'),
         ('broadband', 'speechlike', 'broadband', 'gapped'))

Case = collections.namedtuple('Case', 'name cfg n B kind reduction normalize trim lead trail')


def _lengths(n_fft, hop):
    """the four lengths of audio_cases._analysis_cases"""
    half = n_fft // 2
    return [half + 1, hop * (-(-(half + 2) // hop)) + 1, hop * (-(-n_fft // hop) + 17) + hop - 1, hop * 37]


def _cases():
    cases = []

    def add(cfg, n, kind, trim=0, lead=0, trail=0, normalize=None):
        k = len(cases)
        normalize = (k + k // 8) % 2 if normalize is None else normalize
        n_fft, win, hop = CONFIGS[cfg][:3]
        cases.append(Case('{}:{}/{}/{} n={} {}'.format(k, n_fft, win, hop, n, kind + ('+trim' if trim else '')), cfg, n,
                          BATCHES[k % 3], kind, REDUCTIONS[(k + k // 4) % 4], normalize, trim, lead, trail))

    for i in range(7):
        for j, n in enumerate(_lengths(CONFIGS[i][0], CONFIGS[i][2])):
            # (the alternation would leave the 2048 kernel without a normalised full-scale constant: its DC bin at the clip)
            add(i, n, KINDS[i][j], normalize=1 if (i, j) == (0, 2) else None)
    add(HOP1_CONFIG, 129, 'broadband')
    add(HOP1_CONFIG, 200, 'speechlike')                      # 201 frames
    for j, n in enumerate(_lengths(256, 300)):
        add(WIDE_HOP_CONFIG, n, ('constant', 'broadband', 'speechlike', 'gapped')[j])
    # trim on, one case per kernel: speech between quiet margins, so the frames at the segment's ends reflect about the
    # SEGMENT's ends and must not read the recording's margins
    add(0, 6000, 'speechlike', trim=1, lead=3000, trail=2500)
    add(4, 1600, 'speechlike', trim=1, lead=3000, trail=2500)
    return cases


CASES = _cases()


def config_of(case):
    return CONFIGS[case.cfg]


def frames_of(case):
    """frames with data of an untrimmed recording of the case"""
    return 1 + case.n // CONFIGS[case.cfg][2]


@functools.lru_cache(maxsize=None)
def recordings(index):
    """the B recordings of case `index`, float32, a different signal per recording"""
    c = CASES[index]
    n_fft, _, _, sr = CONFIGS[c.cfg][:4]
    rng = np.random.default_rng(1000 + index)
    out = []
    for b in range(c.B):
        if c.kind == 'broadband':
            y = AC.broadband(rng, c.n, b, float(sr))
        elif c.kind == 'speechlike':
            y = speechlike(rng, c.n, c.lead, c.trail)
        elif c.kind == 'gapped':
            y = gapped(rng, c.n, n_fft)
        else:
            y = constant(c.n) if b == 0 else F32(1.0 - 0.125 * b) * constant(c.n)
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


def param_fields(case):
    """fields of struct tts_feature_params for Engine.feature_params(**...)"""
    n_fft, win, hop, sr, n_mels, fmin, fmax = CONFIGS[case.cfg]
    return dict(n_fft=n_fft, win_length=win, hop_length=hop, sampling_rate=sr, n_mels=n_mels, fmin=fmin, fmax=fmax,
                normalize=case.normalize, reduction=case.reduction, trim=case.trim)


# ----------------------------------------------------------------------------------------------- float64 oracle
Ref = collections.namedtuple('Ref', 'start end Tf T_pad m_lin m_mel empty')


def bank_of(cfg):
    n_fft, _, _, sr, n_mels, fmin, fmax = cfg
    return A.mel_filterbank(sr, n_fft, n_mels, fmin, fmax if fmax > 0 else None)


def segment_of(y, trim, top_db=60, frame_length=2048, hop_length=512):
    if not trim:
        return 0, len(y)
    assert T.threshold_margin(y, top_db, frame_length, hop_length) > 1e-3
    return T.trim_bounds(y, top_db, frame_length, hop_length)


def oracle(y, cfg, reduction, segment=None):
    """float64 magnitudes of one recording (of its `segment`, (start, end), when one is given): m_lin (Tf, F), m_mel
    (Tf, n_mels), with the segment and the frame counts"""
    n_fft, win, hop = cfg[:3]
    s, e = segment or (0, len(y))
    spec = A.stft(np.asarray(y[s:e], dtype=np.float64), n_fft, hop, win, dtype=np.complex128)
    m_lin = np.abs(spec).T
    bank = bank_of(cfg)
    Tf = 1 + (e - s) // hop
    assert m_lin.shape == (Tf, 1 + n_fft // 2)
    return Ref(s, e, Tf, -(-Tf // reduction) * reduction, m_lin, m_lin @ bank.T, ~bank.any(axis=1))


@functools.lru_cache(maxsize=None)
def case_oracle(index):
    c = CASES[index]
    return tuple(oracle(y, CONFIGS[c.cfg], c.reduction, segment_of(y, c.trim)) for y in recordings(index))


# ----------------------------------------------------------------------------------------------- the bound
def _spacing32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def db_interval(m):
    """(lo, hi) dB of every element of the magnitudes m (T, C): f(max(m - d_t, 0)) .. f(m + d_t), f = magnitude_to_decibel in
    float64, each widened by one float32 ulp of the dB value"""
    d = ANALYSIS_TOL * m.max(axis=1, keepdims=True)
    lo = A.magnitude_to_decibel(np.maximum(m - d, 0.0))
    hi = A.magnitude_to_decibel(m + d)
    return lo - _spacing32(lo), hi + _spacing32(hi)


def _normalize_widened(db, ref_db, max_db, sign):
    ref, rng = float(F32(ref_db)), abs(float(F32(ref_db))) + abs(float(F32(max_db)))
    q = (db - ref) / rng
    v = A.normalize_decibel(db, ref, float(F32(max_db)))
    scale = np.maximum(np.abs(v), np.minimum(np.maximum(np.abs(q), 1.0), 2.0))
    return np.clip(v + sign * 2.0 * _spacing32(scale), 0.0, 1.0)


def value_interval(m, normalize, ref_db, max_db):
    """-> (lo, hi, half-width in dB) of the row values of the magnitudes m (T, C)"""
    lo, hi = db_interval(m)
    half = 0.5 * (hi - lo)
    if normalize:
        lo, hi = _normalize_widened(lo, ref_db, max_db, -1.0), _normalize_widened(hi, ref_db, max_db, +1.0)
    return lo, hi, half


def feat_db32(x, normalize, ref_db, max_db):
    """the dB and normalisation lines as feat_db (features.hip) writes them: float32 magnitude, the logarithm in float64 and
    rounded once, the normalisation in float32 with range = |ref| + |max| formed in float32"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        db = (20.0 * np.log10(np.maximum(F32(1e-5), x).astype(np.float64))).astype(np.float32)
        if not normalize:
            return db
        rng = np.abs(F32(ref_db)) + np.abs(F32(max_db))
        return np.clip(F32(1.0) + (db - F32(ref_db)) / rng, F32(0.0), F32(1.0)).astype(np.float32)


def floor_image(normalize, ref_db, max_db):
    """the float32 image of -100 dB (of a zero magnitude)"""
    return feat_db32(np.zeros(1, np.float32), normalize, ref_db, max_db)[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def implied_magnitude(v, normalize, ref_db, max_db):
    v = np.asarray(v, dtype=np.float64)
    if normalize:
        v = (v - 1.0) * (abs(float(F32(ref_db))) + abs(float(F32(max_db)))) + float(F32(ref_db))
    return np.power(10.0, v / 20.0)


def check_rows(mel, lin, ref, normalize, label, consts=CONSTS, constant_dc=False):
    """Hold one recording's rows -- mel (T_pad, n_mels), lin (T_pad, F) float32 -- to the interval and to the exact checks.
    Returns a list of violations (empty: passes) and a dict of diagnostics: per row kind the share of elements whose
    half-width exceeds INFORMATIVE_DB, and the worst |implied magnitude - m| / d_t over the others."""
    bad, info = [], {}
    mel, lin = np.asarray(mel), np.asarray(lin)
    if mel.shape != (ref.T_pad, ref.m_mel.shape[1]) or lin.shape != (ref.T_pad, ref.m_lin.shape[1]):
        return ['{}: shapes {} {} for T_pad {}'.format(label, mel.shape, lin.shape, ref.T_pad)], info
    silent = ref.m_lin.max(axis=1) == 0.0
    for name, got, m, (ref_db, max_db) in (('mel', mel, ref.m_mel, consts[:2]), ('lin', lin, ref.m_lin, consts[2:])):
        g = got[:ref.Tf]
        lo, hi, half = value_interval(m, normalize, ref_db, max_db)
        with np.errstate(invalid='ignore'):
            out = ~((g >= lo) & (g <= hi))
            if normalize:
                out |= ~((g >= 0.0) & (g <= 1.0))
        if out.any():
            t, c = np.argwhere(out)[0]
            bad.append('{} {}: {} of {} values outside the interval, first at frame {} channel {}: {!r} not in [{!r}, {!r}]'
                       .format(label, name, int(out.sum()), out.size, t, c, float(g[t, c]), lo[t, c], hi[t, c]))
        fl = _bits(floor_image(normalize, ref_db, max_db))
        if (_bits(g[silent]) != fl).any():
            bad.append('{} {}: an all-zero frame is not the image of -100 dB'.format(label, name))
        if name == 'mel' and (_bits(g[:, ref.empty]) != fl).any():
            bad.append('{} mel: an empty band is not the image of -100 dB'.format(label))
        if _bits(got[ref.Tf:]).any():
            bad.append('{} {}: a reduction padding row is not 0'.format(label, name))
        if name == 'lin' and constant_dc and normalize and (_bits(g[:, 0]) != _bits(F32(1.0))).any():
            bad.append('{} lin: the DC bin of the full-scale constant is not exactly 1.0'.format(label))
        # diagnostics
        d = ANALYSIS_TOL * m.max(axis=1, keepdims=True)
        inf = (half <= INFORMATIVE_DB) & (m - d > 1e-5) & np.isfinite(g)
        if normalize:
            v = A.normalize_decibel(A.magnitude_to_decibel(m), float(F32(ref_db)), float(F32(max_db)))
            inf &= (v > 1e-6) & (v < 1.0 - 1e-6) & (g > 0.0) & (g < 1.0)
        info[name + '_wide_share'] = float(np.mean(half > INFORMATIVE_DB))
        ratio = 0.0
        if inf.any():
            with np.errstate(over='ignore'):
                ratio = float(np.max((np.abs(implied_magnitude(g, normalize, ref_db, max_db) - m) / np.maximum(d, 1e-300))[inf]))
        info[name + '_ratio'] = ratio
    return bad, info


def check_case(index, outputs, label=None):
    """outputs: per recording (mel (T_red, n_mels r), lin (T_red, F r)), as Engine.extract_features returns them"""
    c = CASES[index]
    n_fft, n_mels = CONFIGS[c.cfg][0], CONFIGS[c.cfg][4]
    refs = case_oracle(index)
    assert len(outputs) == len(refs)
    bad, infos = [], []
    for b, ((mel, lin), ref) in enumerate(zip(outputs, refs)):
        v, info = check_rows(np.asarray(mel).reshape(-1, n_mels), np.asarray(lin).reshape(-1, 1 + n_fft // 2), ref, c.normalize,
                             '{} b{}'.format(label or c.name, b), constant_dc=(c.kind == 'constant' and b == 0))
        bad += v
        infos.append(info)
    return bad, infos


# ----------------------------------------------------------------------------------------------- float32 restatement
def features32(y, cfg, reduction, normalize, segment, consts=CONSTS):
    """audio_cases.stft32 / magnitude32 / mel32 on the segment, then feat_db32, then the reduction padding:
    -> (mel (T_pad, n_mels), lin (T_pad, F), m_mel32 (Tf, n_mels), m_lin32 (Tf, F))"""
    n_fft, win, hop, sr, n_mels, fmin, fmax = cfg
    s, e = segment
    S = AC.stft32(np.array(y[s:e], dtype=np.float32)[None], n_fft, win, hop)
    m_lin = AC.magnitude32(S, 1.0)
    m_mel = AC.mel32(m_lin, sr, n_fft, n_mels, fmin, fmax if fmax > 0 else None)
    m_lin, m_mel = m_lin[0].T, m_mel[0].T
    mel = feat_db32(m_mel, normalize, consts[0], consts[1])
    lin = feat_db32(m_lin, normalize, consts[2], consts[3])
    pad = -(-m_lin.shape[0] // reduction) * reduction - m_lin.shape[0]
    return np.pad(mel, [[0, pad], [0, 0]]), np.pad(lin, [[0, pad], [0, 0]]), m_mel, m_lin
