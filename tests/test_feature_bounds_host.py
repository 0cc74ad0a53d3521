"""CPU: the element-by-element bound of feature_cases.py is FAIR on the inputs the GPU test uses, and it has teeth.

Fairness: a float32 restatement of the feature pass (torch.stft on the CPU, a float32 filter bank product, the dB and
normalisation lines written as feat_db writes them) runs over every case of feature_cases.CASES -- the very recordings of
test_gpu_feature_bounds.py.  Its magnitudes stay within a QUARTER of d_t = 1e-5 max(m[t, :]) of the float64 oracle, element
by element, and its rows pass the interval and the exact checks.  Plain float32 arithmetic therefore has a fourfold margin:
a kernel that misses the bound is wrong, not unlucky.

Teeth: each of a list of deliberately wrong float64 restatements must violate the interval or an exact check on at least
one case of the table.  The float32 log10 among them lies inside the interval everywhere -- 20 log10f(x) differs from the
float64 evaluation by about one float32 ulp of the dB value, and the bound widens by one such ulp on top of at least
8.7e-5 dB from d_t -- and is caught by the exact checks alone: numpy's float32 log10 of the floor magnitude gives
-100.00001 dB where the float64 one, rounded once, gives -100.
"""
import numpy as np
import pytest

import feature_cases as FC
from oracle import audio_oracle as A

F32 = np.float32
N = len(FC.CASES)


# ----------------------------------------------------------------------------------------------- the table itself
def test_table_covers_what_the_kernels_can_get_wrong():
    fast = [c for c in FC.CASES if FC.config_of(c)[0] == 2048]
    slow = [c for c in FC.CASES if FC.config_of(c)[0] != 2048]
    assert {FC.config_of(c)[0] for c in slow} == {256, 512, 1024, 4096}
    for group in (fast, slow):
        plain = [c for c in group if not c.trim]
        assert any(FC.frames_of(c) % c.reduction == 0 and c.reduction > 1 for c in plain)     # no padding row
        assert any(FC.frames_of(c) % c.reduction != 0 for c in plain)
        assert {c.reduction for c in group} == set(FC.REDUCTIONS) and {c.B for c in group} == set(FC.BATCHES)
        assert {c.normalize for c in group} == {0, 1} and sum(c.trim for c in group) == 1
        assert {c.kind for c in group} == {'broadband', 'speechlike', 'gapped', 'constant'}
        assert any(c.kind == 'constant' and c.normalize for c in group)
        assert any(c.kind == 'gapped' and c.normalize for c in group) and any(c.kind == 'gapped' and not c.normalize for c in group)
    # feat2048_kernel deals 8 rows to a workgroup: a batch whose row count leaves a partly filled one
    assert any(sum(r.T_pad for r in FC.case_oracle(FC.CASES.index(c))) % 8 for c in fast)
    assert {FC.config_of(c)[:3] + (c.n,) for c in FC.CASES} >= {(256, 200, 1, 129), (256, 200, 1, 200)}
    assert max(r.Tf for i in range(N) for r in FC.case_oracle(i)) == 201
    assert max(r.Tf for i, c in enumerate(FC.CASES) if c.cfg != FC.HOP1_CONFIG for r in FC.case_oracle(i)) <= 42
    assert any(FC.config_of(c)[2] > FC.config_of(c)[0] for c in FC.CASES)
    # the compact filter bank writes an empty band as lo = hi = 0
    assert (~FC.bank_of(FC.CONFIGS[FC.EMPTY_BAND_CONFIG]).any(axis=1)).sum() >= 1
    for i, c in enumerate(FC.CASES):
        refs = FC.case_oracle(i)
        if c.kind == 'gapped':      # frames of exact zeros, and frames near the floor
            assert all((r.m_lin.max(axis=1) == 0).any() for r in refs), c.name
            assert all((r.m_lin[r.m_lin.max(axis=1) > 0] < 1e-4).any() for r in refs), c.name
        if c.trim:                  # quiet margins on both sides of the segment
            ys = FC.recordings(i)
            assert all(r.start > FC.config_of(c)[0] // 2 and len(y) - r.end > FC.config_of(c)[0] // 2 for r, y in zip(refs, ys))


def test_constants_at_the_floor_and_at_the_clip():
    m, M, l, L = FC.CONSTS
    assert FC.floor_image(0, m, M) == F32(-100.0) and FC.floor_image(0, l, L) == F32(-100.0)
    assert FC.floor_image(1, m, M) == 0.0 and FC.floor_image(1, l, L) == 0.0
    # the full-scale constant: DC = sum of the periodic hann = win / 2, far above the clip at 1
    assert FC.feat_db32(F32(100.0), 1, l, L) == F32(1.0)


# ----------------------------------------------------------------------------------------------- fairness
@pytest.mark.parametrize('index', range(N))
def test_float32_restatement_is_within_a_quarter_of_the_bound(index):
    c = FC.CASES[index]
    worst = 0.0
    for b, (y, ref) in enumerate(zip(FC.recordings(index), FC.case_oracle(index))):
        mel, lin, m_mel, m_lin = FC.features32(y, FC.config_of(c), c.reduction, c.normalize, (ref.start, ref.end))
        for name, m32, m in (('mel', m_mel, ref.m_mel), ('lin', m_lin, ref.m_lin)):
            d = FC.ANALYSIS_TOL * m.max(axis=1, keepdims=True)
            err = np.abs(m32.astype(np.float64) - m)
            assert not err[(d == 0).ravel()].any(), '{} b{} {}: an all-zero frame is not zero in float32'.format(c.name, b, name)
            ratio = float((err / np.where(d == 0, 1.0, d)).max())
            worst = max(worst, ratio)
            assert ratio <= FC.HOST_MARGIN, (c.name, b, name, ratio)
        bad, info = FC.check_rows(mel, lin, ref, c.normalize, '{} b{}'.format(c.name, b), constant_dc=(c.kind == 'constant' and b == 0))
        assert not bad, bad
        print('f32 {} b{}: share of elements wider than {} dB: mel {:.1%} lin {:.1%}; implied-magnitude ratio mel {:.3f} lin {:.3f}'
              .format(c.name, b, FC.INFORMATIVE_DB, info['mel_wide_share'], info['lin_wide_share'], info['mel_ratio'], info['lin_ratio']))
        if c.kind == 'broadband':
            assert info['mel_wide_share'] <= 0.10 and info['lin_wide_share'] <= 0.10, (c.name, b, info)
    print('f32 {}: worst |m32 - m| / d_t {:.4f}'.format(c.name, worst))


# ----------------------------------------------------------------------------------------------- mutants
def restate64(y, cfg, c, seg, window='periodic', shift=0, pad='reflect', mel_ref=None, fmax_off=0.0, drop_last_bin=False,
              floor=1e-5, clip_hi=True, log32=False, mel_late=False):
    """The feature pass in float64, written out (not through the oracle's stft) so that each step can be got wrong:
    -> (mel (T_pad, n_mels), lin (T_pad, F)) float32"""
    n_fft, win, hop, sr, n_mels, fmin, fmax = cfg
    s, e = seg
    y64 = np.concatenate([np.asarray(y, dtype=np.float64), np.zeros(shift)])
    x = y64[s + shift:e + shift]
    half = n_fft // 2
    if pad == 'zero':
        xp = np.pad(x, half, mode='constant')
    else:
        xp = np.pad(x, half, mode='reflect')
        if pad == 'recording':          # the recording's own samples where it has some, the reflection elsewhere
            for i in range(1, half + 1):
                if s - i >= 0:
                    xp[half - i] = y64[s - i]
                if e - 1 + i < len(y):
                    xp[half + len(x) - 1 + i] = y64[e - 1 + i]
    k = np.arange(win, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (win if window == 'periodic' else win - 1))
    w = A.pad_center(w, n_fft)
    Tf = 1 + len(x) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(Tf)[:, None]
    mag = np.abs(np.fft.rfft(xp[idx] * w[None, :], axis=1))
    bank = A.mel_filterbank(sr, n_fft, n_mels, fmin, (fmax if fmax > 0 else sr / 2.0) - fmax_off)
    if drop_last_bin:
        bank = bank.copy()
        for row in bank:
            nz = np.flatnonzero(row)
            if len(nz):
                row[nz[-1]] = 0.0
    mel = mag @ bank.T
    if mel_late:
        mel = np.concatenate([mel[:1], mel[:-1]])

    def rows(m, ref_db, max_db):
        m = np.maximum(floor, m)
        db = (F32(20.0) * np.log10(m.astype(np.float32))).astype(np.float64) if log32 else 20.0 * np.log10(m)
        if c.normalize:
            ref, mx = float(F32(ref_db)), float(F32(max_db))
            db = np.maximum(1.0 + (db - ref) / (abs(ref) + abs(mx)), 0.0)
            if clip_hi:
                db = np.minimum(db, 1.0)
        return np.pad(db.astype(np.float32), [[0, -(-Tf // c.reduction) * c.reduction - Tf], [0, 0]])

    m_ref, m_max, l_ref, l_max = FC.CONSTS
    return rows(mel, m_ref if mel_ref is None else mel_ref, m_max), rows(mag, l_ref, l_max)


def _violations(index, **mutation):
    c = FC.CASES[index]
    bad = []
    for b, (y, ref) in enumerate(zip(FC.recordings(index), FC.case_oracle(index))):
        mel, lin = restate64(y, FC.config_of(c), c, (ref.start, ref.end), **mutation)
        bad += FC.check_rows(mel, lin, ref, c.normalize, '{} b{}'.format(c.name, b), constant_dc=(c.kind == 'constant' and b == 0))[0]
    return bad


def test_the_correct_float64_restatement_passes_every_case():
    for index in range(N):
        assert not _violations(index), FC.CASES[index].name


MUTANTS = {
    'a symmetric hann window': dict(window='symmetric'),
    'a segment taken one sample late': dict(shift=1),
    'zero padding in place of reflection': dict(pad='zero'),
    "the recording's samples read beyond a trimmed segment": dict(pad='recording'),
    'mel_ref_db 6.0 in place of 6.02': dict(mel_ref=6.0),
    'fmax 50 Hz low (7950 for 8000)': dict(fmax_off=50.0),
    'a mel band without its last bin': dict(drop_last_bin=True),
    'a magnitude floor of 1e-4': dict(floor=1e-4),
    'the clip at 1 missing': dict(clip_hi=False),
    'the mel row of frame t written to frame t + 1': dict(mel_late=True),
    'a log10 evaluated in float32': dict(log32=True),
}


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_mutant_is_caught(mutant):
    caught = {}
    for index in range(N):
        bad = _violations(index, **MUTANTS[mutant])
        if bad:
            caught[FC.CASES[index].name] = bad[0]
    print('mutant "{}": caught on {} of {} cases'.format(mutant, len(caught), N))
    for name, first in list(caught.items())[:3]:
        print('   ', first)
    assert caught, 'mutant "{}" passes the interval and the exact checks on every case of the table'.format(mutant)
    # a mutant of the model's own configuration must not need an exotic one to show
    if mutant not in ("the recording's samples read beyond a trimmed segment", 'the clip at 1 missing', 'a magnitude floor of 1e-4',
                      'a log10 evaluated in float32'):
        assert any(FC.CASES[i].cfg == 0 and FC.CASES[i].name in caught for i in range(N)), \
            'mutant "{}" is caught only on {}'.format(mutant, sorted(caught))
