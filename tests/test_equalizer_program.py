"""The host side of the equaliser (csrc/equalizer_plan.h: the constants, the cut of a row into segments and tiles, the workspace
sizes, the recurrence, the transition and the chain, the designs and profiles, and the argument checks of tts_equalize and
tts_set_equalizer) as a stand-alone host program: tests/equalizer_check.cpp with its own main, compiled as plain C++ -- with
AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing preloaded) --
and run.  What it prints is held against tests/equalizer_oracle.py here: every integer exactly, every double of the recurrence bit
for bit (they travel as hex floats).  No GPU, nothing loaded into Python."""
import numpy as np

import equalizer_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals

KNOWN = np.array([0.5, 0.25, -0.125, -0.5, 0.25, 1.0, -2.0, 1.0, -1.5, 0.5625, 0.75, 0.0, -0.75, 0.25, -0.5]).reshape(3, 5)


def sample(i):
    return np.float32(((i * 37) % 101 - 50) / 64.0)


def test_equalizer_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('equalizer_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'cut', 'ws', 'M', 'end', 'row', 'design', 'refuse', 'profile', 'check')}
    c = kinds['consts'][0]
    assert [int(v) for v in c[:6]] == [O.MAX_SECTIONS, O.SEG, O.TILE_SEGS, O.UTTS, O.SR_MIN, O.SR_MAX] == [8, 256, 64, 64, 8000, 192000]
    assert [float.fromhex(v) for v in c[6:12]] == [O.F_MIN, O.F_MAX, O.Q_MIN, O.Q_MAX, O.GAIN_MIN, O.GAIN_MAX] == [1e-4, 0.49, 0.1, 30.0, -40.0, 24.0]
    assert int(c[12]) == O.lds_bytes() <= 80 * 1024 and int(c[13]) == O.SEG + 1

    lengths = [1, 255, 256, 257, 16383, 16384, 16385, 275000, 2147483647]
    assert [int(r[0]) for r in kinds['cut']] == lengths
    for n, segs, last, tiles in (tuple(int(v) for v in r) for r in kinds['cut']):
        assert (segs, last, tiles) == (O.segments(n), O.segment_len(n, O.segments(n) - 1), O.tiles(n)), n
    assert [tuple(int(v) for v in r[1:4]) for r in kinds['cut'][:7]] == [(1, 1, 1), (1, 255, 1), (1, 256, 1), (2, 1, 1), (64, 255, 1), (64, 256, 1),
                                                                        (65, 1, 2)]
    assert len(kinds['ws']) == len(lengths) * 3
    for n, S, state, trans in (tuple(int(v) for v in r) for r in kinds['ws']):
        assert (state, trans) == (O.state_doubles(n, S), O.transition_doubles(S)) == (O.segments(n) * 2 * S, 4 * S * S)

    # the recurrence, bit for bit
    M = O.transition(KNOWN)
    assert len(kinds['M']) == 36
    for r, j, v in kinds['M']:
        assert float.fromhex(v) == M[int(r), int(j)], (r, j)
    x = np.array([sample(i) for i in range(600)], np.float32)
    end = O.end_state(KNOWN, x[:O.SEG])
    assert [float.fromhex(v) for _r, v in kinds['end']] == list(end)
    want = O.equalize(x, KNOWN)
    got = np.array([float.fromhex(v) for _i, v in kinds['row']], np.float64)
    assert len(got) == 600 and np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))

    # the designs: the same formulas in numpy; the libraries' tan, pow and sqrt may differ in their last bit
    assert len(kinds['design']) == 7
    for r in kinds['design']:
        kind, sr = int(r[0]), int(r[1])
        f0, q, g = (float.fromhex(v) for v in r[2:5])
        np.testing.assert_allclose([float.fromhex(v) for v in r[5:]], O.design(kind, sr, f0, q, g), rtol=1e-13, atol=0)
    answers = {name: int(code) for name, code in kinds['refuse']}
    assert len(answers) == 14
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 2 if name.endswith('_above') else 1), (name, code)
    assert len(kinds['profile']) == 15
    for name, sr, code, n in kinds['profile']:
        fits = O.profile_fits(name, int(sr))
        assert int(code) == (0 if fits else 2) and int(n) == (len(O.PROFILES[name]) if fits else 0), (name, sr)
    assert {name for name, sr, code, _n in kinds['profile'] if int(code)} == {'bright', 'warm'}      # 6 kHz does not fit 8000 Hz

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 6 + 5 + 3 + 2 + 3 + 7 + 1 + 4 + 2
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
