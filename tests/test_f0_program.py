"""The host side of F0 tracking (csrc/f0_plan.h: the frame count, the first sample of a frame, the frames a workgroup owns and its
LDS bytes, the lag bounds and the argument checks of tts_f0 and tts_f0_compare) as a stand-alone host program: tests/f0_check.cpp
with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked
statically: the program needs nothing preloaded) -- and run.  What it prints is held against tests/f0_oracle.py here, every
integer exactly.  No GPU, nothing loaded into Python."""
import f0_oracle as Y
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_f0_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('f0_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'frames', 'first', 'group', 'groups', 'lags', 'f0_check')}
    max_w, max_lag, lanes, slots, max_group, utts, budget = (int(v) for v in kinds['consts'][0])
    assert (max_w, max_lag) == (2048, 1024) and lanes * slots == max_lag and max_group >= 1 and utts >= 1 and budget <= 64 * 1024

    assert len(kinds['frames']) >= 35
    for n, hop, T in kinds['frames']:
        assert int(T) == Y.frames(int(n), int(hop))
    assert len(kinds['first']) == 4 * 2 * 3 * 3
    for t, hop, W, hi, s0 in kinds['first']:
        assert int(s0) == Y.first_sample(int(t), int(hop), int(W), int(hi))
    assert len(kinds['group']) == 6 * 9 * 8
    for W, hi, hop, frames, span, nbytes, stride, sl in (tuple(int(v) for v in g) for g in kinds['group']):
        assert span == W + hi + (frames - 1) * hop and stride >= hi + 1 and stride % 2 == 1
        assert nbytes == 8 * (span + 2 * frames * stride) <= budget
        assert frames == max_group or 8 * (span + hop + 2 * (frames + 1) * stride) > budget
        assert sl == -(-hi // lanes)
    for T, frames, g in kinds['groups']:
        assert int(g) == -(-int(T) // int(frames))
    assert len(kinds['lags']) == 30
    for sr, f, lo, hi in kinds['lags']:
        want_lo, _ = Y.lag_bounds(float(sr), 1.0, float(f))
        _, want_hi = Y.lag_bounds(float(sr), float(f), float(f))
        assert (int(lo), int(hi)) == (want_lo, want_hi), (sr, f)

    answers = {name: int(code) for name, code in kinds['f0_check']}
    assert len(answers) == 23
    for name, code in answers.items():
        want = 0 if name.startswith('legal') else 2 if name.endswith('_above') else 1
        assert code == want, (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
