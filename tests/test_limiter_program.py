"""The host side of the limiter stage (csrc/limiter_plan.h: the taps, the ceiling's float, the tile and halo arithmetic of the
kernels, the sliding minimum by doubling and the argument checks of tts_true_peak, tts_limit and tts_set_limiter) as a stand-alone
host program: tests/limiter_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host
compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held against
tests/limiter_oracle.py here.  No GPU, nothing loaded into Python."""
import numpy as np

import limiter_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_limiter_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('limiter_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'taps', 'ceiling', 'tile', 'tiles', 'check')}
    max_l, phases, n_taps, before, after, beta, utts, tile, lanes = kinds['consts'][0]
    assert (int(max_l), int(phases), int(n_taps), int(before), int(after)) == (O.MAX_LOOKAHEAD, O.PHASES, O.TAPS, O.BEFORE, O.AFTER)
    assert float(beta) == O.BETA and int(tile) == O.TILE and int(utts) >= 1 and int(tile) % int(lanes) == 0

    # the taps: numpy's design to a few ulp (another libm, another Bessel series); phase 0 the impulse exactly
    taps = np.array([[float(v) for v in r[1:]] for r in kinds['taps']])
    assert taps.shape == (O.PHASES, O.TAPS) and [int(r[0]) for r in kinds['taps']] == list(range(O.PHASES))
    assert np.array_equal(taps[0], np.eye(O.TAPS)[O.BEFORE])
    # (a tap is below 1 and takes a sine, a square root, two Bessel values, a product and two quotients on either side: 16 ulp of
    #  the binade under 1, 16 * 2 ** -53, is room for a few ulp each)
    assert np.abs(taps - O.design()).max() < 16 * 2.0 ** -53

    assert len(kinds['ceiling']) == 8
    for c, cf in kinds['ceiling']:
        assert np.float32(cf) == O.ceiling_float(float(c)), (c, cf)

    assert len(kinds['tile']) == 10
    for L, xc, rc, lds, steps, span in (tuple(int(v) for v in r) for r in kinds['tile']):
        assert rc == O.TILE + 4 * L and xc == rc + O.BEFORE + O.AFTER and lds == 8 * (xc + 2 * rc) <= 160 * 1024
        assert span == 1 << steps and span <= 2 * L + 1 < 2 * span
    assert [tuple(int(v) for v in r) for r in kinds['tiles']] == [(1, 1), (2047, 1), (2048, 1), (2049, 2), (2147483647, 1048576)]

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 26
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
