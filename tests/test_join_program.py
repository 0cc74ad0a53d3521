"""The host side of the join (csrc/join_plan.h: the checks of an edit list, where every piece lands, the fade of its edges, the
entries the kernel is handed and the cut into launches) as a stand-alone host program: tests/join_check.cpp with its own main,
compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the
program needs nothing preloaded) -- and run.  What it prints is held against tests/join_oracle.py, every integer exactly.  No GPU,
nothing loaded into Python."""
import join_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_join_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('join_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'launches', 'list', 'piece', 'n_out', 'entry', 'room', 'check')}
    per_launch, max_pieces, max_fade, threads, tile = (int(v) for v in kinds['consts'][0])
    assert (per_launch, max_pieces, max_fade, threads, tile) == (128, 4096, 1 << 20, 128, 512) and tile == 4 * threads
    assert {int(p): int(n) for p, n in kinds['launches']} == {P: -(-P // 128) for P in (1, 127, 128, 129, 4096)}

    # the layout of every list: offsets, fades and lengths are the oracle's integers
    assert [r[0] for r in kinds['list']] == ['one', 'last_gap_ignored', 'crossfade', 'groups', 'short_fades', 'large_gap']
    for name, B, N, fade, P, G in kinds['list']:
        got = [[int(v) for v in r[1:]] for r in kinds['piece'] if r[0] == name]
        assert [r[0] for r in got] == list(range(int(P)))
        pieces, groups = [tuple(r[1:5]) for r in got], [r[5] for r in got]
        offsets, n_out, f = O.plan(pieces, groups, int(fade))
        assert [r[6] for r in got] == offsets and [r[7] for r in got] == f, name
        assert [int(r[2]) for r in kinds['n_out'] if r[0] == name] == n_out and len(n_out) == int(G), name
        assert all(0 <= row < int(B) and first >= 0 and first + count <= int(N) for row, first, count, _gap in pieces)
        room = next(r[1:] for r in kinds['room'] if r[0] == name)
        assert [int(v) for v in room] == [int(any(n > min(n_out[0], 2 ** 31 - 1) for n in n_out)), 1], name
    large = [int(r[2]) for r in kinds['n_out'] if r[0] == 'large_gap']
    assert large == [12 + 2 * (2 ** 31 - 1)]                      # a length beyond int32 is counted, not wrapped
    # the kernel's entries of 'groups' at N_out = 40: flat starts g * N_out + o, the overlap with the predecessor inside a group only
    assert [[int(v) for v in r] for r in kinds['entry']] == [[0, 0, 0], [1, 7, 6], [2, 40, 0], [3, 80, 0], [4, 92, 1], [5, 95, 0]]

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 28
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    want = {'count=%d' % n: LENGTH_REFUSAL.format(name='count', b=3, n=n, bound='N - first', hi=1992) for n in (0, -1, 1993)}
    want.update({
        'room': 'N_out = 8 is below n_out[1] = 9', 'samples': '',
        'samples5': 'G * N_out = 10737418235 output samples are more than 2^33 = 8589934592',
        'G7': '7 groups of 6 pieces: no group is empty', 'Gmax': '2147483647 groups of 6 pieces: no group is empty',
        'null': 'a NULL pointer (pieces, group and n_out are required)',
        'B0': 'need B, N, P, G >= 1', 'N0': 'need B, N, P, G >= 1', 'P0': 'need B, N, P, G >= 1', 'G0': 'need B, N, P, G >= 1',
        'fade-1': 'fade < 0',
        'fade_max': 'fade = 1048577 is larger than tts_join_max_fade() = 1048576',
        'pieces_max': '4097 pieces are more than tts_join_max_pieces() = 4096',
        'row-1': 'row[2] = -1 is not in 0 .. B - 1 = 4', 'row5': 'row[2] = 5 is not in 0 .. B - 1 = 4',
        'first-1': 'first[1] = -1 is not in 0 .. N - 1 = 2002', 'first2003': 'first[1] = 2003 is not in 0 .. N - 1 = 2002',
        'group_start': 'group[0] = 1: the groups start at 0',
        'group_back': 'group[3] = 0 follows 1: the groups are non-decreasing and none is empty',
        'group_skip': 'group[2] = 2 follows 0: the groups are non-decreasing and none is empty',
        'group_end': 'group[5] = 2: the last group is G - 1 = 3',
        'gap': 'gap[0] = -7 overlaps more than min(f[0], f[1]) = 6 samples',
        'gap_short': 'gap[3] = -2 overlaps more than min(f[3], f[4]) = 1 samples',
    })
    assert refusals == want
