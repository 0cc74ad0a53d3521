"""The host side of the resampler (csrc/resample_plan.h: the filter design, the lengths, the constants of a ratio, the position
of an output and the argument checks of tts_resample) as a stand-alone host program: tests/resample_check.cpp with its own main,
compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the
program needs nothing preloaded) -- and run.  What it prints is held against the numpy oracle here: lengths and integers exactly,
table values to 1e-13 of max |win|.  No GPU, nothing loaded into Python."""
import numpy as np

import resample_oracle as R
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals

TABLE_TOL = 1e-13


def test_resample_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('resample_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('len', 'win', 'consts', 'tab', 'phase')}
    assert len(kinds['len']) == 8 * 11 and len(kinds['consts']) == 8 and len(kinds['phase']) == 8 * 11 and len(kinds['tab']) > 8 * 40
    for n, rho, valid, length in kinds['len']:
        assert int(valid) == R.resampled_valid(int(n), float(rho)) and int(length) == R.resampled_length(int(n), float(rho)), (n, rho)
    base = R.half_window()
    top = np.abs(base).max()
    assert len(kinds['win']) > 300
    for j, v in kinds['win']:
        assert abs(float(v) - base[int(j)]) <= TABLE_TOL * top, (j, v, base[int(j)])
    for rho, scale, inc, step, taps_max, row in kinds['consts']:
        want = R.consts(float(rho))
        assert (float(scale), int(step), float(inc)) == (float(want[0]), want[1], float(want[2])), rho
        assert int(taps_max) == R.NWIN // want[1] and int(row) == -(-int(taps_max) // 8) * 8
    windows = {}
    for rho, off, i, w, d in kinds['tab']:
        rho = float(rho)
        if rho not in windows:
            windows[rho] = R.window(rho)
        win, delta = windows[rho]
        j = int(off) + int(i) * R.consts(rho)[1]
        scale_top = np.abs(win).max()
        assert abs(float(w) - win[j]) <= TABLE_TOL * scale_top and abs(float(d) - delta[j]) <= TABLE_TOL * scale_top, (rho, off, i)
    for rho, n_in, t, m, off0, eta0, taps0, off1, eta1, taps1 in kinds['phase']:
        wm, (o0, e0, k0), (o1, e1, k1) = R.phase(int(t), int(n_in), float(rho))
        assert (int(m), int(off0), int(taps0), int(off1), int(taps1)) == (int(wm), int(o0), int(k0), int(o1), int(k1)), (rho, t)
        assert float(eta0) == float(e0) and float(eta1) == float(e1), (rho, t)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='n', hi=100) for n in (0, -1, 101)}
