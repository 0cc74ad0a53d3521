"""What the segment-wise stages share (csrc/segments.h: the order of a list's rows, the cut into launches, a launch's tile numbering
and segment_find, the bisection their kernels run) as a stand-alone host program: tests/segments_check.cpp with its own main,
compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the program
needs nothing preloaded) -- and run.  The program holds segment_find against a linear scan itself; what it prints is held against
a scan of the printed tables here, and the refusals' texts are fixed once.  No GPU, nothing loaded into Python."""
from host_checks import build_and_run, length_refusals

TABLES = ['one', 'two', 'two_first_empty', 'two_last_empty', 'runs', 'n63', 'n63_last_empty', 'n64_ones', 'n64', 'n64_first_empty',
          'n64_middle_empty', 'n64_last_empty', 'n64_only_first', 'n64_only_17', 'n64_only_last', 'n130']


def test_segments_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('segments_check.cpp', tmp_path)[0])
    kinds = {}
    for r in rows:
        kinds.setdefault(r[0], []).append(r[1:])
    assert [int(v) for v in kinds['consts'][0]] == [64, 4096]
    assert [tuple(int(v) for v in r) for r in kinds['launches']] == [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 64)]

    # every launch of every table: its tiles are numbered entry after entry, and every tile was found at the entry that owns it
    launches = {}
    for r in kinds['launch']:
        launches.setdefault(r[0], []).append([int(v) for v in r[1:]])
    assert list(launches) == TABLES
    found = {}
    for name, l, tile, q in kinds['own']:
        found.setdefault((name, int(l)), []).append((int(tile), int(q)))
    shapes = {}
    for name, per_launch in launches.items():
        for at, (l, n, tiles, *own) in enumerate(per_launch):
            assert l == at and len(own) == n and sum(own) == tiles and tiles >= 1, (name, l)
            owners = [q for q, k in enumerate(own) for _ in range(k)]
            assert found[(name, l)] == list(enumerate(owners)), (name, l)
            shapes.setdefault(name, []).append(own)
    assert [len(v) for v in shapes['n130']] == [64, 64, 2]
    # the tables the kernels meet: 1, 2, 63 and 64 entries; entries without a tile first, in the middle, last and in runs; one owner
    assert {len(v[0]) for v in shapes.values()} == {1, 2, 10, 63, 64}
    assert shapes['two_first_empty'] == [[0, 4]] and shapes['two_last_empty'] == [[4, 0]] and shapes['runs'] == [[2, 0, 0, 0, 3, 0, 0, 1, 0, 0]]
    assert shapes['n63'][0][0] == 0 and shapes['n63_last_empty'][0][-1] == 0 and shapes['n64_ones'] == [[1] * 64]
    assert shapes['n64_first_empty'][0][0] == 0 and shapes['n64_last_empty'][0][-1] == 0 and shapes['n64_middle_empty'][0][30:34] == [0] * 4
    for name, at in (('n64_only_first', 0), ('n64_only_17', 17), ('n64_only_last', 63)):
        assert shapes[name] == [[5 if q == at else 0 for q in range(64)]]

    # the shared refusals, in the library's words
    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 11
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert {k: v for k, v in msgs.items() if not k.startswith('legal')} == {
        'segments_max': '4097 segments are more than toy_max_segments() = 4096',
        'rows_over_segments': '7 rows of 6 segments: no row is without a segment',
        'length': 'n_toy[1] = 41 is not in 1 .. W = 40',
        'row_start': 'row of segment 0 is 1: the rows start at 0',
        'row_back': 'row of segment 4 is 0 and follows 1: the rows are non-decreasing and none is without a segment',
        'row_skip': 'row of segment 3 is 2 and follows 0: the rows are non-decreasing and none is without a segment',
        'row_negative': 'row of segment 2 is -1 and follows 0: the rows are non-decreasing and none is without a segment',
        'row_end': 'row of segment 5 is 1: the last row is B - 1 = 2',
        'room': 'W_out = 8 is below n_out[1] = 9',
        'room_max': 'W_out = 1073741825 is above 2^30 = 1073741824',
    }
    assert all(v == '' for k, v in msgs.items() if k.startswith('legal')) and sum(k.startswith('legal') for k in msgs) == 3
