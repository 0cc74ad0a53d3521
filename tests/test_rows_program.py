"""The row rules every ragged stage shares (csrc/lengths.h: the refusal of a length outside ``lo`` .. ``hi`` for the lower bounds 0 and
1, the in/out pair of the stages that filter rows, a launch's chunk of lengths and its longest) as a stand-alone host program:
tests/rows_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their
runtimes, linked statically -- and run.  The texts are fixed here once, in the library's words.  No GPU, nothing loaded into Python."""
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals

ALIGNED = 'wav and out must be 4-byte aligned'
OVERLAP = 'out overlaps wav without being equal to it'


def test_rows_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('rows_check.cpp', tmp_path)[0])

    # the bounded refusal: -1, 0, 1, N and N + 1 at index 1 of three, for both lower bounds
    refusal = 'n_samples[1] = {} is not in {} .. N = 5000'.format
    assert refusal(0, 1) == LENGTH_REFUSAL.format(name='n_samples', b=1, n=0, bound='N', hi=5000)
    assert {k: v for k, v in msgs.items() if k.startswith('lo')} == {
        'lo0_-1': refusal(-1, 0), 'lo0_0': '', 'lo0_1': '', 'lo0_5000': '', 'lo0_5001': refusal(5001, 0),
        'lo1_-1': refusal(-1, 1), 'lo1_0': refusal(0, 1), 'lo1_1': '', 'lo1_5000': '', 'lo1_5001': refusal(5001, 1)}
    assert msgs['default_lo'] == 'n_frames[0] = 0 is not in 1 .. T = 3'

    # the in/out pair: equal or disjoint, exactly adjacent on either side is disjoint, and the alignment comes first
    pairs = {k: v for k, v in msgs.items() if not k.startswith('lo') and k != 'default_lo'}
    assert pairs == {
        'legal_equal': '', 'legal_adjacent_behind': '', 'legal_adjacent_ahead': '',
        'inside_front': OVERLAP, 'inside_back': OVERLAP, 'inside_ahead': OVERLAP, 'inside_behind': OVERLAP,
        'misaligned_wav': ALIGNED, 'misaligned_out': ALIGNED, 'misaligned_and_overlapping': ALIGNED}

    # fill_lengths: the chunk it writes (zeros behind nb) and the longest length it returns
    fills = {r[1]: [int(v) for v in r[2:]] for r in rows if r[0] == 'fill'}
    assert fills == {'full': [9, 9, 2, 7, 3], 'short_last': [8, 3, 8, 0, 0], 'null': [100, 100, 100, 0, 0]}
    assert len(rows) == len(fills)
