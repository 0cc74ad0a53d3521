"""The host side of the prosody warp (csrc/warp_plan.h: the checks of a segment list, the output frames of every segment and row,
the cut into launches and tiles) as a stand-alone host program: tests/warp_check.cpp with its own main, compiled as plain C++ --
with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing
preloaded) -- and run.  What it prints is held against tests/warp_oracle.py here.  No GPU, nothing loaded into Python."""
import warp_oracle as O
from host_checks import build_and_run, length_refusals


def test_warp_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('warp_check.cpp', tmp_path)[0])
    kinds = {}
    for r in rows:
        kinds.setdefault(r[0], []).append(r[1:])
    per_launch, most, threads, tile, bins, step_min, step_max = (int(v) for v in kinds['consts'][0])
    assert (per_launch, most, tile, step_min, step_max) == (O.SEGMENTS_PER_LAUNCH, O.MAX_SEGMENTS, O.TILE, O.STEP_MIN, O.STEP_MAX)
    assert threads % tile == 0 and bins % (threads // tile) == 0
    assert [tuple(int(v) for v in r) for r in kinds['launches']] == [(S, O.launches(S)) for S in (1, 63, 64, 65, 4096)] == \
        [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 64)]

    # the counts: the oracle's, at both ends of the step's range, and with frames * 65536 one below, at and one above a multiple of step
    seen = set()
    for frames, step, c in ((int(v) for v in r) for r in kinds['count']):
        assert c == O.count(frames, step), (frames, step)
        assert (c - 1) * step < frames * 65536 <= c * step
        rest = (frames * 65536) % step
        seen.add((step in (step_min, step_max), 'at' if rest == 0 else 'above' if rest == 1 else 'below' if rest == step - 1 else 'between'))
    assert {(True, 'at'), (True, 'between'), (False, 'at'), (False, 'above'), (False, 'below'), (False, 'between')} <= seen
    assert len(kinds['count']) >= 80

    # every list: the lengths and the cut
    assert [r[0] for r in kinds['list']] == ['one', 'pauses', 'seam', 'straddle', 'rows65']
    for name, B, T, S, T_out in ((r[0], *(int(v) for v in r[1:])) for r in kinds['list']):
        n_frames = [int(r[2]) for r in kinds['frames'] if r[0] == name]
        seg = [(int(r[2]), int(r[3]), int(r[4]), int(r[5]), int(r[6]), float(r[7])) for r in kinds['seg'] if r[0] == name]
        got_counts = [int(r[8]) for r in kinds['seg'] if r[0] == name]
        assert len(seg) == S and len(n_frames) == B
        why, n_out, counts = O.plan(seg, B, T, n_frames)
        assert why is None and counts == got_counts, name
        assert [int(r[2]) for r in kinds['n_out'] if r[0] == name] == n_out, name
        assert T_out >= max(n_out) and O.room(n_out, T_out) is None
        cut = O.cut(seg, counts, T_out)
        entries = [tuple(int(v) for v in r[1:]) for r in kinds['entry'] if r[0] == name]
        assert len(entries) == S and len(cut) == O.launches(S)
        o, s = 0, 0
        for launch, tiles in enumerate(cut):
            first = 0
            for t in tiles:
                last = s + 1 == S or seg[s + 1][0] != seg[s][0]
                speech = seg[s][2] > 0
                assert entries[s] == (s, launch, first, t, o, counts[s] if speech else 0, T_out - o if last else counts[s]), (name, s)
                first += t
                o = 0 if last else o + counts[s]
                s += 1
            assert [int(r[2]) for r in kinds['tiles'] if r[0] == name][launch] == first, (name, launch)
    # the seam: TILE - 1, TILE and TILE + 1 frames are 1, 1 and 2 tiles
    seam = {int(r[7]): int(r[4]) for r in kinds['entry'] if r[0] == 'seam'}
    assert (seam[tile - 1], seam[tile], seam[tile + 1], seam[4 * 65 + 3]) == (1, 1, 2, 5)

    # every refusal, in the library's words (the oracle's plan makes the same ones: test_prosody_host.py)
    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 35
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert sum(name.startswith('legal') for name in answers) == 5
    assert msgs == {
        'null': 'a NULL pointer (segments and n_out are required)',
        'B0': 'need B, T, S >= 1', 'T0': 'need B, T, S >= 1', 'S0': 'need B, T, S >= 1',
        'segments_max': '4097 segments are more than tts_warp_max_segments() = 4096',
        'rows_over_segments': '10 rows of 9 segments: no row is without a segment',
        'Bmax': '2147483647 rows of 9 segments: no row is without a segment',
        'n_frames=0': 'n_frames[1] = 0 is not in 1 .. T = 40', 'n_frames=-1': 'n_frames[1] = -1 is not in 1 .. T = 40',
        'n_frames=41': 'n_frames[1] = 41 is not in 1 .. T = 40',
        'row_start': 'row of segment 0 is 1: the rows start at 0',
        'row_back': 'row of segment 4 is 0 and follows 1: the rows are non-decreasing and none is without a segment',
        'row_skip': 'row of segment 6 is 2 and follows 0: the rows are non-decreasing and none is without a segment',
        'row_end': 'row of segment 8 is 1: the last row is B - 1 = 2',
        'row_negative': 'row of segment 6 is -1 and follows 0: the rows are non-decreasing and none is without a segment',
        'frames-1': 'segment 2 has a negative length (frames -1, pause 0)',
        'pause-2': 'segment 3 has a negative length (frames 0, pause -2)',
        'both': 'segment 2 is both speech (12 frames) and a pause (3 frames)',
        'neither': 'segment 4 is neither speech nor a pause (frames and pause are 0)',
        'past_the_row': 'segment 1 reads frames 21 .. 40 of row 0, which has 0 .. 39',
        'past_n_frames': 'segment 7 reads frames 7 .. 7 of row 1, which has 0 .. 6',
        'first-1': 'segment 2 reads frames -1 .. 10 of row 0, which has 0 .. 39',
        'first_max': 'segment 1 reads frames 2147483647 .. 2147483666 of row 0, which has 0 .. 39',
        'step_low': 'segment 2 has step 16383, which is not in 16384 .. 262144',
        'step_high': 'segment 2 has step 262145, which is not in 16384 .. 262144',
        'step0': 'segment 2 has step 0, which is not in 16384 .. 262144',
        'gain_nan': 'segment 6 has a gain that is not finite or lies outside 0 .. 16',
        'gain_inf': 'segment 6 has a gain that is not finite or lies outside 0 .. 16',
        'gain_negative': 'segment 6 has a gain that is not finite or lies outside 0 .. 16',
        'gain_high': 'segment 6 has a gain that is not finite or lies outside 0 .. 16',
        'room': 'T_out = 8 is below n_out[1] = 9',
        'room_max': 'T_out = 1073741825 is above 2^30 = 1073741824',
    }
