"""The host side of the compressor (csrc/compressor_plan.h: the constants, the workspace sizes, the detector, both chains, the gain
computer, the designs and profiles, and the argument checks of tts_compress and tts_set_compressor) as a stand-alone host program:
tests/compressor_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has
their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held against
tests/compressor_oracle.py here: every integer exactly, every double of the detector and the chains bit for bit (they travel as hex
floats), the output to the bound of compressor_cases (libm's log10 and pow against numpy's).  No GPU, nothing loaded into Python."""
import numpy as np

import compressor_cases as C
import compressor_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals

KNOWN = O.Params(-20.0, 0.25, 6.0, 3.0, 0.875, 0.9375)


def sample(i):
    return np.float32(np.float32(((i * 37) % 101 - 50) / 64.0) * np.float32(1.0 if i % 700 < 350 else 0.03125))


def test_compressor_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('compressor_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'ws', 'coef', 'row', 'chain', 'r', 'rhard', 'design', 'refuse', 'profile', 'check')}
    c = kinds['consts'][0]
    assert [float.fromhex(v) for v in c[:6]] == [O.THRESHOLD_MIN, O.THRESHOLD_MAX, O.KNEE_MAX, O.MAKEUP_MIN, O.MAKEUP_MAX, O.MS_MAX] == \
        [-80.0, 0.0, 40.0, -24.0, 24.0, 10000.0]
    assert int(c[6]) == O.UTTS == 64
    lengths = [1, 255, 256, 257, 16384, 16385, 275000, 2147483647]
    assert [tuple(int(v) for v in r) for r in kinds['ws']] == [(n, O.state_doubles(n), O.partials(n)) for n in lengths]
    assert [tuple(int(v) for v in r[1:]) for r in kinds['ws'][:6]] == [(2, 1), (2, 1), (2, 1), (4, 1), (128, 1), (130, 2)]

    k = O.coef(KNOWN)
    assert [float.fromhex(v) for v in kinds['coef'][0]] == [k.s1, k.bA, k.AA, k.AR, 0.0]
    assert 0 < k.AA < k.AR < 1

    # the row: the envelope bit for bit, the output to the bound, the special positions bit for bit
    x = np.array([sample(i) for i in range(1500)], np.float32)
    x[700], x[701], x[702] = np.nan, np.inf, -0.0
    w = O.compress(x, KNOWN)
    got = np.array([float.fromhex(v) for _i, v, _e in kinds['row']], np.float64)
    env = np.array([float.fromhex(e) for _i, _v, e in kinds['row']], np.float64)
    assert len(got) == 1500 and C.same_doubles(env, w.envelope)
    ok, worst = C.held(got.astype(np.float32), w)
    assert ok and worst <= 1.0, worst
    assert np.sum(w.r < 0) > 300 and np.sum(w.r == 0) > 300                  # the loud stretches are reduced, the quiet ones not
    chain = np.array([[float.fromhex(v) for v in r[1:]] for r in kinds['chain']])
    assert len(chain) == O.segments(1500) - 1 == 5
    for col, name in enumerate('csqt'):
        assert C.same_doubles(chain[:, col], getattr(w, name)[:5]), name

    # the gain computer: computed directly, so -inf gives 0 and not NaN
    for L, r in kinds['r']:
        L, r = float.fromhex(L), float.fromhex(r)
        assert r == float(O.reduction(k, np.float64(L))), L
    assert [float.fromhex(r) for _L, r in kinds['r'][:3]] == [0.0, 0.0, 0.0] and float.fromhex(kinds['r'][3][1]) < 0
    assert float.fromhex(kinds['r'][5][1]) == -0.75 * 3.0 and float.fromhex(kinds['r'][8][1]) == -0.75 * 80.0
    assert [float.fromhex(r) for _L, r in kinds['rhard']] == [0.0, 0.0, -0.5, -20.0]

    # the designs: libm's exp may differ from Python's in its last bit
    assert len(kinds['design']) == 4
    for r in kinds['design']:
        sr, a_ms, r_ms, a, rel = int(r[0]), *(float.fromhex(v) for v in r[1:])
        np.testing.assert_allclose([a, rel], O.design(sr, a_ms, r_ms), rtol=4e-16, atol=0)
    answers = {name: int(code) for name, code in kinds['refuse']}
    assert len(answers) == 6
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 2), name
    assert len(kinds['profile']) == 9
    for r in kinds['profile']:
        np.testing.assert_allclose([float.fromhex(v) for v in r[2:]], O.profile(r[0], int(r[1])), rtol=4e-16, atol=0)

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 5 + 5 + 3 + 2 * 24 + 5
    for name, code in answers.items():
        assert code == (0 if 'legal' in name else 1), (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
