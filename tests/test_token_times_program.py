"""The host side of the timing marks (csrc/token_times_plan.h: the launches a batch is cut into, where the directions of the search
live, the weight of an element, and the argument checks of tts_token_times) as a stand-alone host program:
tests/token_times_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has
their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held against the definition
here, every integer exactly.  No GPU, nothing loaded into Python."""
import numpy as np

import marks_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_token_times_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('token_times_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'record', 'launches', 'dir', 'weight', 'nan', 'check')}
    utts, threads, passes, tokens, jump, per_chunk, dir_lds = (int(v) for v in kinds['consts'][0])
    assert (utts, threads, passes, tokens, jump, per_chunk, dir_lds) == (64, 256, 4, 1024, 15, 2, 32768)
    assert tokens == threads * passes >= 1024
    # the record: 32 bytes, the int64 first, six int32 in the order of the header -- the numpy dtype of the oracle
    size, *offsets = (int(v) for v in kinds['record'][0])
    assert size == O.RECORD.itemsize == 32
    assert tuple(offsets) == tuple(O.RECORD.fields[n][1] for n in ('score',) + O.FIELDS) == (0, 8, 12, 16, 20, 24, 28)

    # two launches per 64 utterances: 1 -> 2, 64 -> 2, 65 -> 4
    launches = {int(b): (int(n), int(c)) for b, n, c in kinds['launches']}
    assert launches == {B: (2 * -(-B // 64), -(-B // 64)) for B in (1, 2, 63, 64, 65, 128, 129, 1000)}
    assert launches[1] == (2, 1) and launches[64] == (2, 1) and launches[65] == (4, 2)

    # a byte of direction per cell in LDS up to 32 KiB, else none of it; two rows of int64 always
    assert len(kinds['dir']) == 6 * 8
    for S, Ts, in_lds, lds in (tuple(int(v) for v in r) for r in kinds['dir']):
        assert in_lds == (1 if S * Ts <= 32768 else 0) and lds == 16 * Ts + (S * Ts if in_lds else 0), (S, Ts)
    at = {(int(r[0]), int(r[1])): int(r[2]) for r in kinds['dir']}
    assert at[(130, 130)] == 1 and at[(130, 300)] == 0 and at[(200, 100)] == 1 and at[(130, 252)] == 1 and at[(130, 253)] == 0

    # the weights are the oracle's
    bits = np.array([int(b, 16) for b, _w in kinds['weight']] + [int(b, 16) for b, _w in kinds['nan']], np.uint32)
    got = [int(w, 16) for _b, w in kinds['weight']] + [int(w, 16) for _b, w in kinds['nan']]
    assert len(got) == 13 + 5 and got == list(O.weights(bits.view(np.float32)))
    assert got[-5:] == [0] * 5 and got[12] == 0x7f800000 and got[6] == 1

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 21
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 2 if name == 'too_wide' else 1), (name, code)
    want = {'n_sent=%d' % n: LENGTH_REFUSAL.format(name='n_sent', b=1, n=n, bound='Ts', hi=92) for n in (0, -1, 93)}
    want.update({'n_steps=%d' % n: LENGTH_REFUSAL.format(name='n_steps', b=2, n=n, bound='n_steps_max', hi=200) for n in (0, -1, 201)})
    want.update({'J=%d' % j: 'max_jump = %d is not in 1 .. 15' % j for j in (0, -1, 16)})
    want['lengths_first'] = LENGTH_REFUSAL.format(name='n_sent', b=0, n=93, bound='Ts', hi=92)
    want['invalid_first'] = 'max_jump = 0 is not in 1 .. 15'
    want['null'] = 'a NULL pointer (alignments, start and stats are required)'
    want['B0'] = 'need B, Ts, n_steps_max >= 1'
    want['too_wide'] = 'Ts = 1025 is above the 1024 tokens of a table'
    assert refusals == want
