"""The host side of the formant-preserving pitch stage (csrc/shift_plan.h: the checks of a segment list, the cut into launches and
tiles, the tables and the LDS of a workgroup) as a stand-alone host program: tests/shift_check.cpp with its own main, compiled as
plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the program needs
nothing preloaded) -- and run.  What it prints is held against tests/shift_oracle.py here.  No GPU, nothing loaded into Python."""
import numpy as np

import shift_oracle as O
from host_checks import build_and_run, length_refusals


def test_shift_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('shift_check.cpp', tmp_path)[0])
    kinds = {}
    for r in rows:
        kinds.setdefault(r[0], []).append(r[1:])
    assert tuple(int(v) for v in kinds['consts'][0]) == (O.SEGMENTS_PER_LAUNCH, O.MAX_SEGMENTS, 512, O.TILE, O.COPY_TILE, O.MAX_ORDER, O.STEP_MIN,
                                                         O.STEP_MAX, O.N_MIN, O.N_MAX) == (64, 4096, 512, 8, 64, 256, 32768, 131072, 128, 2048)
    assert [tuple(int(v) for v in r) for r in kinds['launches']] == [(S, O.launches(S)) for S in (1, 63, 64, 65, 4096)] == \
        [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 64)]
    # the LDS of a workgroup: 8 frames a pass up to N = 1024, 4 at 2048; never above a compute unit's 160 KB
    lds = {(int(r[0]), int(r[1])): (int(r[2]), int(r[3])) for r in kinds['lds']}
    assert lds[(1024, 33)] == (8, 8 * (2112 + 8 * 1032 + 33 * 8) + 4 * 8 * 1032 + 32) and lds[(2048, 256)][0] == 4
    assert max(v[1] for v in lds.values()) == lds[(2048, 256)][1] == 140704 <= 160 * 1024
    # the tables are numpy's to the last bit or one ulp beside it
    for N, j, v in ((int(r[0]), int(r[1]), float.fromhex(r[2])) for r in kinds['ct']):
        assert abs(v - O.cos_table(N)[j]) <= np.spacing(abs(v)), (N, j)
    for Q, q, v in ((int(r[0]), int(r[1]), float.fromhex(r[2])) for r in kinds['lifter']):
        assert abs(v - O.lifter(Q)[q]) <= np.spacing(abs(v)), (Q, q)
    assert float.fromhex(kinds['lifter'][0][2]) == 1.0 and float.fromhex(kinds['ct'][0][2]) == 1.0

    # every list: legal for the oracle, and the oracle's cut
    assert [r[0] for r in kinds['list']] == ['one', 'seam', 'ragged', 'straddle']
    for name, B, F, T, S in ((r[0], *(int(v) for v in r[1:])) for r in kinds['list']):
        n_frames = [int(r[2]) for r in kinds['frames'] if r[0] == name]
        seg = [tuple(int(v) for v in r[2:]) for r in kinds['seg'] if r[0] == name]
        assert len(seg) == S and len(n_frames) == B
        assert O.plan(seg, B, F, T, n_frames, 2) is None, name
        cut = O.cut(seg, T)
        entries = [tuple(int(v) for v in r[1:]) for r in kinds['entry'] if r[0] == name]
        assert len(entries) == S and len(cut) == O.launches(S)
        s = 0
        for launch, owned in enumerate(cut):
            first = 0
            for lead, body, rest in owned:
                assert entries[s] == (s, launch, first, lead, body, rest), (name, s)
                first += lead + body + rest
                s += 1
            assert [int(r[2]) for r in kinds['tiles'] if r[0] == name][launch] == first, (name, launch)
    seam = {int(r[1]): int(r[5]) for r in kinds['entry'] if r[0] == 'seam'}
    assert [seam[s] for s in range(5)] == [1, 1, 2, 1, 3]                    # segments of tile - 1, tile, tile + 1 frames; a copy; 17 frames
    assert len([r for r in kinds['tiles'] if r[0] == 'straddle']) == 2

    # every refusal, in the library's words and in the documented order
    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 44
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert sum(name.startswith('legal') for name in answers) == 5
    assert msgs == {
        'null': 'a NULL pointer (segments are required)',
        'B0': 'need B, T, S >= 1', 'T0': 'need B, T, S >= 1', 'S0': 'need B, T, S >= 1', 'B_before_F': 'need B, T, S >= 1',
        'F_even': 'F = 2048 is not 2^m + 1 with 2^m in 128 .. 2048', 'F_small': 'F = 65 is not 2^m + 1 with 2^m in 128 .. 2048',
        'F_large': 'F = 4097 is not 2^m + 1 with 2^m in 128 .. 2048', 'F_before_order': 'F = 65 is not 2^m + 1 with 2^m in 128 .. 2048',
        'order_low': 'order = 1 is not in 2 .. 256', 'order_high': 'order = 257 is not in 2 .. 256', 'order_half_n': 'order = 65 is not in 2 .. 64',
        'segments_max': '4097 segments are more than tts_shift_max_segments() = 4096', 'order_before_segments_max': 'order = 1 is not in 2 .. 64',
        'rows_over_segments': '10 rows of 4 segments: no row is without a segment',
        'Bmax': '2147483647 rows of 4 segments: no row is without a segment',
        'n_frames=0': 'n_frames[1] = 0 is not in 1 .. T = 200', 'n_frames=-1': 'n_frames[1] = -1 is not in 1 .. T = 200',
        'n_frames=201': 'n_frames[1] = 201 is not in 1 .. T = 200',
        'row_start': 'row of segment 0 is 1: the rows start at 0',
        'row_back': 'row of segment 3 is 0 and follows 1: the rows are non-decreasing and none is without a segment',
        'row_skip': 'row of segment 3 is 2 and follows 0: the rows are non-decreasing and none is without a segment',
        'row_end': 'row of segment 3 is 2: the last row is B - 1 = 3',
        'row_negative': 'row of segment 1 is -1 and follows 0: the rows are non-decreasing and none is without a segment',
        'frames0': 'segment 1 has 0 frames: at least 1 is needed', 'frames-3': 'segment 1 has -3 frames: at least 1 is needed',
        'past_the_row': 'segment 1 covers frames 140 .. 200 of row 0, which has 0 .. 199',
        'past_n_frames': 'segment 2 covers frames 0 .. 41 of row 1, which has 0 .. 40',
        'first-1': 'segment 0 covers frames -1 .. 1 of row 0, which has 0 .. 199',
        'first_max': 'segment 1 covers frames 2147483647 .. 2147483706 of row 0, which has 0 .. 199',
        'overlap': "segment 1 starts at frame 72 of row 0, in front of its predecessor's end 73: the ranges of a row ascend and do not overlap",
        'precedes': "segment 1 starts at frame 10 of row 0, in front of its predecessor's end 73: the ranges of a row ascend and do not overlap",
        'reserved': 'segment 3 has reserved = 1, which must be 0',
        'range_before_reserved': 'segment 3 covers frames 9 .. 9 of row 2, which has 0 .. 8',
        'pitch_low': 'segment 0 has pitch_step 32767, which is not in 32768 .. 131072',
        'pitch_high': 'segment 0 has pitch_step 131073, which is not in 32768 .. 131072',
        'formant_low': 'segment 0 has formant_step 32767, which is not in 32768 .. 131072',
        'formant_high': 'segment 0 has formant_step 131073, which is not in 32768 .. 131072',
        'reserved_before_steps': 'segment 0 has reserved = 7, which must be 0',
    }
    # the oracle's plan makes the same refusals of the same lists (test_shift_host.py holds the library's and the binding's to them)
    ok = [(0, 70, 3, 52016, 65536), (0, 140, 60, 65536, 65536), (1, 0, 41, 52016, 65536), (2, 3, 1, 73562, 73562)]
    assert O.plan(ok, 3, 2049, 200, [200, 41, 9], 64) is None
    assert O.plan(ok[:1] + [(0, 72, 60, 65536, 65536)] + ok[2:], 3, 2049, 200, [200, 41, 9], 64) == msgs['overlap']
    assert O.plan(ok, 3, 129, 200, [200, 41, 9], 65) == msgs['order_half_n']
