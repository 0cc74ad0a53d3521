"""GPU: tts_resample_segments against tests/resample_segments_oracle.py -- every resampled element within resample_oracle.bound
(2^-24 |y| + 2^-36 sum |w| |x|, the project's own bound for this arithmetic), every copy and every zero bit for bit -- on the
ragged batch of resample_cases.py (rows of 5000 floats, NaN at and behind every length); `out` holds a NaN pattern before every
call and lies one float behind an allocation's start in half of them."""
import ctypes

import numpy as np
import pytest

import resample_cases as RC
import resample_oracle as R
import resample_segments_cases as C
import resample_segments_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu


def test_the_constants_and_the_cases(engine):
    assert (engine.resample_segments_tile(), engine.resample_segments_max(), engine.resample_segments_max_ratios()) == \
        (O.TILE, O.MAX_SEGMENTS, O.MAX_RATIOS) == (256, 4096, 16)
    case = C.mixed()
    _why, _n, counts = O.plan(case['segments'], case['B'], C.N, case['n_samples'])
    assert {0, 1, 255, 256, 257} <= set(counts) and max(counts) > 4 * O.TILE
    ratios = {q[3] for q in case['segments']}
    assert ratios == set(RC.RATIOS) and case['segments'][21] == case['segments'][22]
    assert case['segments'][20][1] > case['segments'][21][1]                                                       # out of source order
    assert [len(C.LISTS[k]()['segments']) for k in ('seam65', 'seam130')] == [65, 130]
    rows = [q[0] for q in C.seam130()['segments']]
    assert rows[63] != rows[64] and rows[127] == rows[128]                                                          # a seam between rows, one inside
    assert len({q[3] for q in C.ratios16()['segments'] if q[3] < 1.0}) == 16


@pytest.mark.parametrize('name', list(C.LISTS))
def test_it_is_the_oracle(engine, name):
    H = pkg('_hip')
    case, x = C.inputs(name)
    seg, ns = case['segments'], case['n_samples']
    for extra in (0, 3):                                                        # N_out at and above the longest row
        want = C.oracle(name, extra)
        N_out = want['y'].shape[1]
        for shift in ((0, 1) if extra else (1,)):
            rc, got, around, got_n = C.raw_call(engine, H, x, ns, seg, N_out, shift)
            assert rc == 0, engine.lib.tts_last_error(engine.handle)
            assert got_n.tolist() == want['n_out']
            assert (around == C.NAN_PATTERN).all()                              # the canary: nothing outside out[B][N_out] is written
            assert not (got == C.NAN_PATTERN).any()                             # ... and every element of it is
            C.assert_matches(got, want, (name, extra, shift), R)
    for b, n in enumerate(want['n_out']):
        assert not want['kind'][b, n:].any() and (want['kind'][b, :n] != 0).all()
    if name == 'mixed':
        assert (want['kind'] == O.COPY).any() and (want['bits'][want['kind'] == O.COPY] == 0x7fc12345).any()     # a payload travelled
        assert (want['bits'][want['kind'] == O.COPY] == 0x80000000).any()
    # the binding: a fresh (B, longest) array and the plan's lengths, from a device buffer and from a host array, n_out not asked for
    want = C.oracle(name, 0)
    d = engine.to_device(x)
    try:
        assert engine.resample_segments_plan(x.shape, seg, ns).tolist() == want['n_out']
        for src in (d, x):
            out, got_n = engine.resample_segments(src, seg, ns)
            try:
                assert got_n.tolist() == want['n_out'] and out.shape == want['y'].shape
                C.assert_matches(out.to_host().view(np.uint32), want, (name, 'binding'), R)
            finally:
                out.free()
        rc, got, _a, got_n = C.raw_call(engine, H, x, ns, seg, want['y'].shape[1], 0, want_n=False)
        assert rc == 0 and (got_n == -7).all()
        C.assert_matches(got, want, (name, 'no n_out'), R)
    finally:
        d.free()


@pytest.mark.parametrize('rho', [r for r in RC.RATIOS if r != 1.0], ids=[i for i in RC.RATIO_IDS if i != '1.0'])
def test_one_segment_per_row_is_tts_resample(engine, rho):
    """the containment: (b, 0, n_b, ratio) per row is the bits of tts_resample on the same rows, at N_out below, at and above"""
    x = RC.ragged_batch()
    seg = [(b, 0, n, rho) for b, n in enumerate(RC.RAGGED)]
    d = engine.to_device(x)
    try:
        for N_out in RC.n_out_choices(max(RC.RAGGED), rho)[1:]:
            out, n_out = engine.resample_segments(d, seg, RC.RAGGED, N_out)
            ref = engine.resample(d, rho, RC.RAGGED, N_out)
            try:
                assert n_out.tolist() == [R.resampled_valid(n, rho) for n in RC.RAGGED]
                a, b = out.to_host(), ref.to_host()
                assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            finally:
                out.free()
                ref.free()
    finally:
        d.free()


def test_a_rows_bits_depend_neither_on_the_batch_nor_on_the_launches(engine):
    """row 4's segments of `mixed` alone, behind 70 other segments of a first row (another launch, other tiles), and in the batch"""
    case, x = C.inputs('mixed')
    mine = [q for q in case['segments'] if q[0] == 4]
    whole, _n = engine.resample_segments(x, case['segments'], case['n_samples'])
    alone, n_alone = engine.resample_segments(x[4:5], [(0,) + q[1:] for q in mine], [700])
    filler = [(0, 3 * k, 40, RC.RATIOS[k % 8]) for k in range(70)]
    two, n_two = engine.resample_segments(x[[5, 4]], filler + [(1,) + q[1:] for q in mine], [5000, 700])
    try:
        n = int(n_alone[0])
        assert n == n_two[1] == C.oracle('mixed')['n_out'][4]
        a = whole.to_host().view(np.uint32)[4, :n]
        assert np.array_equal(a, alone.to_host().view(np.uint32)[0, :n]) and np.array_equal(a, two.to_host().view(np.uint32)[1, :n])
    finally:
        for o in (whole, alone, two):
            o.free()


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_a_nan_or_inf_reaches_the_outputs_whose_window_covers_it_and_no_other(engine, value):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((1, 1200)).astype(np.float32)
    at = 600
    x[0, at] = value
    seg = [(0, 0, 1200, RC.RATIOS[2]), (0, 500, 200, 1.0), (0, 300, 600, 2.0), (0, 0, 580, 0.5), (0, 560, 30, 0.25), (0, 610, 500, RC.RATIOS[3])]
    want = O.resample_segments(x, seg)
    mask = (want['lo'][0] <= at) & (at <= want['hi'][0])
    assert mask.sum() > 300 and (~mask).sum() > 1000 and mask[want['kind'][0] == O.COPY].sum() == 1
    out, n_out = engine.resample_segments(x, seg)
    try:
        got = out.to_host()[0]
        assert np.array_equal(~np.isfinite(got), mask)                          # (an Inf's window holds +Inf, -Inf or, where both meet, NaN)
        clean = x.copy()
        clean[0, at] = 0.0
        ref = O.resample_segments(clean, seg)
        C.assert_matches(np.where(mask, 0, got.view(np.uint32))[None], dict(ref, y=np.where(mask, 0.0, ref['y']), bits=np.where(mask, 0, ref['bits'])),
                         'beside the window', R)
    finally:
        out.free()


def test_the_padding_is_never_read_and_the_source_may_be_anything(engine):
    """the same rows with finite garbage behind every length give the same bits as with NaN there"""
    case, x = C.inputs('mixed')
    y = x.copy()
    for b, n in enumerate(case['n_samples']):
        y[b, n:] = 1e30
    a, _n = engine.resample_segments(x, case['segments'], case['n_samples'])
    b, _n = engine.resample_segments(y, case['segments'], case['n_samples'])
    try:
        assert np.array_equal(a.to_host().view(np.uint32), b.to_host().view(np.uint32))
    finally:
        a.free()
        b.free()


def test_refusals_enqueue_nothing_and_a_legal_call_counts_its_launches(engine):
    H = pkg('_hip')
    case, x = C.inputs('mixed')
    ns, seg = case['n_samples'], case['segments']
    N_out = C.oracle('mixed', 3)['y'].shape[1]
    edit = lambda s, j, v: [tuple(v if (a, b) == (s, j) else y for b, y in enumerate(q)) for a, q in enumerate(seg)]
    many = [(0, 0, 1, 1.0)] * 4097
    seventeen = [(0, 0, 10, 2.0 ** (-(k + 1) / 48.0)) for k in range(17)]
    bad_ratio = 'segment 13 has a ratio that is not finite or lies outside [0.25, 4]'
    cases = [
        (dict(S=0), 'need B, n, S, N_out >= 1'),
        (dict(B=0), 'need B, n, S, N_out >= 1'),
        (dict(N_out=0), 'need B, n, S, N_out >= 1'),
        (dict(segments=many, B=1, n_samples=[40]), '4097 segments are more than tts_resample_segments_max() = 4096'),
        (dict(B=29), '29 rows of 28 segments: no row is without a segment'),
        (dict(n_samples=[1, 2, 63, 64, 5001, 5000]), 'n_samples[4] = 5001 is not in 1 .. n = 5000'),
        (dict(n_samples=[1, 2, 63, 64, 700, 0]), 'n_samples[5] = 0 is not in 1 .. n = 5000'),
        (dict(segments=edit(0, 0, 1)), 'row of segment 0 is 1: the rows start at 0'),
        (dict(segments=edit(7, 0, 1)), 'row of segment 7 is 1 and follows 2: the rows are non-decreasing and none is without a segment'),
        (dict(segments=[q for q in seg if q[0] != 3]), 'row of segment 9 is 4 and follows 2: the rows are non-decreasing and none is without a segment'),
        (dict(segments=[q for q in seg if q[0] != 5]), 'row of segment 19 is 4: the last row is B - 1 = 5'),
        (dict(segments=edit(13, 2, 0)), 'segment 13 has 0 samples: at least 1 is needed'),
        (dict(segments=edit(13, 2, 513)), 'segment 13 reads samples 188 .. 700 of row 4, which has 0 .. 699'),
        (dict(segments=edit(13, 1, -1)), 'segment 13 reads samples -1 .. 510 of row 4, which has 0 .. 699'),
        (dict(segments=edit(13, 3, 0.2)), bad_ratio), (dict(segments=edit(13, 3, 4.5)), bad_ratio),
        (dict(segments=edit(13, 3, float('nan'))), bad_ratio), (dict(segments=edit(13, 3, float('inf'))), bad_ratio),
        (dict(segments=[q + (7,) if s == 2 else q for s, q in enumerate(seg)]), 'segment 2 has reserved = 7, which must be 0'),
        (dict(segments=seventeen, B=1, n_samples=[700]),
         'segment 16 brings distinct ratio below 1 number 17: a call takes tts_resample_segments_max_ratios() = 16'),
        (dict(N_out=N_out - 4), 'N_out = {} is below n_out[5] = {}'.format(N_out - 4, N_out - 3)),
    ]
    d = engine.to_device(x)
    engine.set_option('profile', 1)
    try:
        engine.profile_reset()
        for kw, text in cases:
            rc, got, around, _n = C.raw_call(engine, H, x, kw.get('n_samples', ns), kw.get('segments', seg), kw.get('N_out', N_out), 0, kw.get('S'), kw.get('B'))
            assert rc == H.TTS_ERR_INVALID, (kw, rc)
            assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'resample_segments: ' + text, kw
            assert (got == C.NAN_PATTERN).all() and (around == C.NAN_PATTERN).all()
        # NULL pointers, n < 1 and a misaligned buffer: the library itself
        q = C.segment_array(H, seg)
        pn = np.asarray(ns, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out = engine.empty((6, N_out))
        null = 'a NULL pointer (wav, segments and out are required)'
        try:
            for args, text in (((None, 6, C.N, pn, q.ctypes.data, len(q), N_out, out.data_ptr(), None), null),
                               ((d.data_ptr(), 6, C.N, pn, None, len(q), N_out, out.data_ptr(), None), null),
                               ((d.data_ptr(), 6, C.N, pn, q.ctypes.data, len(q), N_out, None, None), null),
                               ((d.data_ptr(), 6, 0, pn, q.ctypes.data, len(q), N_out, out.data_ptr(), None), 'need B, n, S, N_out >= 1'),
                               ((d.data_ptr(), 6, C.N, pn, q.ctypes.data, len(q), (1 << 30) + 1, out.data_ptr(), None),
                                'N_out = 1073741825 is above 2^30 = 1073741824'),
                               ((d.data_ptr(), 6, C.N, pn, q.ctypes.data, len(q), N_out, out.data_ptr() + 2, None), 'the buffers must be 4-byte aligned')):
                assert engine.lib.tts_resample_segments(engine.handle, *args) == H.TTS_ERR_INVALID
                assert (engine.lib.tts_last_error(engine.handle) or b'').decode() == 'resample_segments: ' + text
        finally:
            out.free()
        with pytest.raises(ValueError, match='segment 13 has a ratio'):
            engine.resample_segments(d, edit(13, 3, 0.2), ns)
        assert engine.profile_get('resample') == (0.0, 0)
        # legal calls: the launches the plan predicts, under the stage "resample"
        engine.resample_segments(d, seg, ns)[0].free()
        assert engine.profile_get('resample')[1] == O.launches(len(seg)) == 1
        for name, launches in (('seam65', 2), ('seam130', 3)):
            other, y = C.inputs(name)
            engine.profile_reset()
            engine.resample_segments(y, other['segments'], other['n_samples'])[0].free()
            assert engine.profile_get('resample')[1] == O.launches(len(other['segments'])) == launches
        engine.profile_reset()
        engine.resample_segments(x[:1], [(0, 0, 1, 0.25)], [1])[0].free()      # a list that owns one zero
        assert engine.profile_get('resample')[1] == 1 and engine.profile_get('warp') == (0.0, 0)
    finally:
        engine.set_option('profile', 0)
        d.free()


def test_more_ratios_than_the_handle_keeps_tables_for(engine):
    """40 ratios below 1 over three calls, more than the 32 tables a handle keeps: the cache is emptied between calls, never under
    one, and the first call's result comes out again afterwards, bit for bit"""
    rng = np.random.default_rng(40)
    x = rng.standard_normal((1, 700)).astype(np.float32)
    lists = [[(0, 20 * k, 200, 0.5 + 0.01 * (16 * c + k) + 0.001) for k in range(16 if c < 2 else 8)] for c in range(3)]
    first, _n = engine.resample_segments(x, lists[0])
    try:
        want = O.resample_segments(x, lists[0])
        C.assert_matches(first.to_host().view(np.uint32), want, 'first', R)
        for seg in lists[1:]:
            out, _n = engine.resample_segments(x, seg)
            got = out.to_host().view(np.uint32)
            out.free()
            C.assert_matches(got, O.resample_segments(x, seg), 'later', R)
        again, _n = engine.resample_segments(x, lists[0])
        try:
            assert np.array_equal(again.to_host().view(np.uint32), first.to_host().view(np.uint32))
        finally:
            again.free()
    finally:
        first.free()
