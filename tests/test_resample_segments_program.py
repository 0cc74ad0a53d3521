"""The host side of the segment-wise resampler (csrc/resample_segments_plan.h: the checks of a segment list, the output samples
of every segment and row, the cut into launches and tiles) as a stand-alone host program: tests/resample_segments_check.cpp with
its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked
statically: the program needs nothing preloaded) -- and run.  What it prints is held against tests/resample_segments_oracle.py
here.  No GPU, nothing loaded into Python."""
import resample_oracle as R
import resample_segments_oracle as O
from host_checks import build_and_run, length_refusals


def test_resample_segments_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('resample_segments_check.cpp', tmp_path)[0])
    kinds = {}
    for r in rows:
        kinds.setdefault(r[0], []).append(r[1:])
    assert tuple(int(v) for v in kinds['consts'][0]) == (O.SEGMENTS_PER_LAUNCH, O.MAX_SEGMENTS, O.MAX_RATIOS, O.TILE) == (64, 4096, 16, 256)
    assert [tuple(int(v) for v in r) for r in kinds['launches']] == [(S, O.launches(S)) for S in (1, 63, 64, 65, 4096)] == \
        [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 64)]

    # the counts: a copy keeps its samples, anything else is resampy's truncated product
    assert len(kinds['count']) == 64
    for samples, ratio, c in ((int(r[0]), float.fromhex(r[1]), int(r[2])) for r in kinds['count']):
        assert c == O.count(samples, ratio) == (samples if ratio == 1.0 else int(samples * ratio)), (samples, ratio)
    # the LDS of a tile: the windows of 256 outputs, about 6 KB at the lowest ratio
    for ratio, span in ((float.fromhex(r[0]), int(r[1])) for r in kinds['span_max']):
        _scale, step, inc = R.consts(ratio)
        assert span == int(255 * inc) + 2 + 2 * (R.NWIN // step)
    assert int(kinds['span_max'][0][1]) * 4 == 6136

    # every list: the lengths and the cut
    assert [r[0] for r in kinds['list']] == ['one', 'mixed', 'straddle', 'rows65']
    for name, B, n, S, N_out in ((r[0], *(int(v) for v in r[1:])) for r in kinds['list']):
        n_samples = [int(r[2]) for r in kinds['samples'] if r[0] == name]
        seg = [(int(r[2]), int(r[3]), int(r[4]), float.fromhex(r[5])) for r in kinds['seg'] if r[0] == name]
        got_counts = [int(r[6]) for r in kinds['seg'] if r[0] == name]
        assert len(seg) == S and len(n_samples) == B
        why, n_out, counts = O.plan(seg, B, n, n_samples)
        assert why is None and counts == got_counts, name
        assert [int(r[2]) for r in kinds['n_out'] if r[0] == name] == n_out, name
        assert N_out >= max(max(n_out), 1) and O.room(n_out, N_out) is None
        below = []
        for q in seg:
            if q[3] < 1.0 and q[3] not in below:
                below.append(q[3])
        assert [tuple(int(v) for v in r[1:]) for r in kinds['ratios'] if r[0] == name] == [(len(below), int(any(q[3] > 1.0 for q in seg)))]
        cut = O.cut(seg, counts, N_out)
        entries = [tuple(int(v) for v in r[1:]) for r in kinds['entry'] if r[0] == name]
        assert len(entries) == S and len(cut) == O.launches(S)
        s, covered = 0, {}
        for launch, owned in enumerate(cut):
            first = 0
            for o, span, tiles in owned:
                tab = -1 if seg[s][3] == 1.0 else 0 if seg[s][3] > 1.0 else below.index(seg[s][3]) + 1
                assert entries[s] == (s, launch, first, tiles, o, counts[s], span, tab), (name, s)
                covered[seg[s][0]] = covered.get(seg[s][0], 0) + span
                first += tiles
                s += 1
            assert [int(r[2]) for r in kinds['tiles'] if r[0] == name][launch] == first, (name, launch)
        assert covered == {b: N_out for b in range(B)}, name                       # every element of out has one owner
    mixed = {int(r[1]): (int(r[4]), int(r[6])) for r in kinds['entry'] if r[0] == 'mixed'}
    assert [mixed[s] for s in (0, 1, 2, 3, 4)] == [(1, 255), (1, 256), (2, 257), (1, 255), (0, 0)]       # tiles of 255, 256, 257 and no sample
    # a launch's LDS is that of its largest segment that produces a sample: 0.5 in `mixed` (its 0.25 segments produce none), 3.5 in
    # the second launch of `straddle` (row 2 at 0.3 produces none)
    assert [int(r[3]) for r in kinds['tiles'] if r[0] == 'mixed'] == [int(255 * 2.0) + 2 + 2 * 128]
    straddle = [int(r[3]) for r in kinds['tiles'] if r[0] == 'straddle']
    assert len(straddle) == 2 and straddle[1] == int(255 / 3.5) + 2 + 2 * 64

    # every refusal, in the library's words
    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 34
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert sum(name.startswith('legal') for name in answers) == 4
    bad_ratio = 'segment 3 has a ratio that is not finite or lies outside [0.25, 4]'
    assert msgs == {
        'null': 'a NULL pointer (segments and n_out are required)',
        'B0': 'need B, n, S >= 1', 'n0': 'need B, n, S >= 1', 'S0': 'need B, n, S >= 1',
        'segments_max': '4097 segments are more than tts_resample_segments_max() = 4096',
        'rows_over_segments': '11 rows of 10 segments: no row is without a segment',
        'Bmax': '2147483647 rows of 10 segments: no row is without a segment',
        'n_samples=0': 'n_samples[1] = 0 is not in 1 .. n = 700', 'n_samples=-1': 'n_samples[1] = -1 is not in 1 .. n = 700',
        'n_samples=701': 'n_samples[1] = 701 is not in 1 .. n = 700',
        'row_start': 'row of segment 0 is 1: the rows start at 0',
        'row_back': 'row of segment 7 is 0 and follows 1: the rows are non-decreasing and none is without a segment',
        'row_skip': 'row of segment 6 is 2 and follows 0: the rows are non-decreasing and none is without a segment',
        'row_end': 'row of segment 9 is 2: the last row is B - 1 = 3',
        'row_negative': 'row of segment 6 is -1 and follows 0: the rows are non-decreasing and none is without a segment',
        'samples0': 'segment 2 has 0 samples: at least 1 is needed',
        'samples-3': 'segment 2 has -3 samples: at least 1 is needed',
        'past_the_row': 'segment 1 reads samples 189 .. 700 of row 0, which has 0 .. 699',
        'past_n_samples': 'segment 7 reads samples 33 .. 64 of row 1, which has 0 .. 63',
        'first-1': 'segment 2 reads samples -1 .. 512 of row 0, which has 0 .. 699',
        'first_max': 'segment 1 reads samples 2147483647 .. 2147484158 of row 0, which has 0 .. 699',
        'ratio_low': bad_ratio, 'ratio_high': bad_ratio, 'ratio_nan': bad_ratio, 'ratio_inf': bad_ratio, 'ratio_negative': bad_ratio,
        'reserved': 'segment 4 has reserved = 1, which must be 0',
        'ratio_before_reserved': bad_ratio,
        'ratios_max': 'segment 19 brings distinct ratio below 1 number 17: a call takes tts_resample_segments_max_ratios() = 16',
        'reserved_before_ratios_max': 'segment 20 has reserved = 5, which must be 0',
        'room': 'N_out = 8 is below n_out[1] = 9',
        'room_max': 'N_out = 1073741825 is above 2^30 = 1073741824',
    }
    # the oracle's plan makes the same refusals of the same lists (test_resample_segments_host.py holds the binding's to them)
    ok = [(0, 100, 255, 1.0), (0, 188, 512, 0.5), (1, 0, 64, 4.0)]
    assert O.plan(ok, 2, 700, [700, 64])[0] is None
    assert O.plan([(0, 189, 512, 0.5)], 1, 700)[0] == 'segment 0 reads samples 189 .. 700 of row 0, which has 0 .. 699'
    assert O.plan([(0, 0, 5, 0.5, 1)], 1, 700)[0] == 'segment 0 has reserved = 1, which must be 0'
    assert O.room([5, 9], 8) == msgs['room'] and O.room([5, 9], (1 << 30) + 1) == msgs['room_max']
