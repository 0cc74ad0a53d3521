"""The host side of the attention diagnostics (csrc/alignment_plan.h: the launches a batch is cut into, how a wave covers a row,
the keys an argmax is decided by, and the argument checks of tts_alignment_stats and tts_text_lengths) as a stand-alone host
program: tests/alignment_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host
compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held against
the definition here, every integer exactly.  No GPU, nothing loaded into Python."""
import numpy as np

import alignment_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_alignment_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('alignment_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'record', 'launches', 'blocks', 'cover', 'key', 'nan', 'check', 'text')}
    utts, per_block, per_chunk = (int(v) for v in kinds['consts'][0])
    assert (utts, per_block, per_chunk) == (64, 4, 2)
    # the record: 56 bytes, twelve int32 in the order of the header, the double at 48 -- the numpy dtype of the oracle
    size, at_first, at_skipped, at_reserved, at_focus = (int(v) for v in kinds['record'][0])
    assert size == O.RECORD.itemsize == 56 and at_first == 0
    assert (at_skipped, at_reserved, at_focus) == tuple(O.RECORD.fields[n][1] for n in ('skipped', 'reserved', 'focus_sum')) == (40, 44, 48)

    # two launches per 64 utterances: 64 -> 2, 65 -> 4
    launches = {int(b): (int(n), int(c)) for b, n, c in kinds['launches']}
    assert launches == {B: (2 * -(-B // 64), -(-B // 64)) for B in (1, 2, 63, 64, 65, 128, 129, 1000)}
    assert launches[64] == (2, 1) and launches[65] == (4, 2)
    assert {int(s): int(n) for s, n in kinds['blocks']} == {S: -(-S // 4) for S in (1, 2, 3, 4, 5, 40, 200, 1000)}

    assert len(kinds['cover']) == 15 * 4
    for Ts, mis, head, vecs, tail in (tuple(int(v) for v in r) for r in kinds['cover']):
        assert head == min(Ts, (4 - mis) % 4) and vecs == (Ts - head) // 4 and tail == Ts - head - 4 * vecs, (Ts, mis)

    # the keys order float32 values as np.argmax does
    keys = [(np.array([int(b, 16)], np.uint32).view(np.float32)[0], int(k, 16)) for b, k in kinds['key']]
    assert len(keys) == 11
    for (v0, k0), (v1, k1) in zip(keys[:-1], keys[1:]):
        assert (k1 == k0) if v1 == v0 else (v1 > v0 and k1 > k0), (v0, v1)
    assert all(int(k, 16) == 0xffffffff for _b, k in kinds['nan']) and len(kinds['nan']) == 5

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 16
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert {name: int(code) for name, code in kinds['text']} == {'legal': 0, 'null': 1, 'B0': 1, 'Ts0': 1}
    want = {'n_sent=%d' % n: LENGTH_REFUSAL.format(name='n_sent', b=1, n=n, bound='Ts', hi=92) for n in (0, -1, 93)}
    want.update({'n_steps=%d' % n: LENGTH_REFUSAL.format(name='n_steps', b=2, n=n, bound='n_steps_max', hi=200) for n in (0, -1, 201)})
    want['both'] = LENGTH_REFUSAL.format(name='n_sent', b=0, n=93, bound='Ts', hi=92)
    want['null'] = 'a NULL pointer (alignments and stats are required)'
    want['B0'] = 'need B, Ts, n_steps_max >= 1'
    want['text_null'] = 'a NULL pointer (ids and n_sent are required)'
    want['text_B0'] = 'need B, Ts >= 1'
    assert refusals == want
