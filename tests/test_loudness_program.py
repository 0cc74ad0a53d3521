"""The host side of the loudness stage (csrc/loudness_plan.h: the cut of an utterance into steps, segments and blocks, the
workspace it asks for and the argument checks of tts_loudness, tts_loudness_normalize and tts_set_loudness) as a stand-alone host
program: tests/loudness_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host
compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held against
tests/loudness_oracle.py here, every integer exactly.  No GPU, nothing loaded into Python."""
import loudness_oracle as O
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_loudness_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('loudness_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'cut', 'blocks', 'check')}
    lo, hi, segs, utts, z_abs, rel = kinds['consts'][0]
    assert (int(lo), int(hi), int(segs)) == (O.SR_MIN, O.SR_MAX, O.SEGS) and int(utts) >= 1
    # the gate constants: the plan header's literals are the oracle's, and the absolute one is the double nearest the formula
    assert float(z_abs) == O.Z_ABS == 10.0 ** ((-70.0 + 0.691) / 10.0) and float(rel) == O.REL == 0.1

    assert len(kinds['cut']) == 12
    for row in kinds['cut']:
        sr, s, c = (int(v) for v in row[:3])
        assert (s, c) == (O.step(sr), O.segment(sr))
        assert [int(v) for v in row[3:]] == O.segment_lengths(sr)
    assert [int(v) for v in [r for r in kinds['cut'] if r[0] == '22050'][0][3:]] == [276] * 7 + [273]
    assert len(set([r for r in kinds['cut'] if r[0] == '16000'][0][3:])) == 1          # equal segments

    assert len(kinds['blocks']) == 12 * 11
    for sr, n, K, J, read, ws in (tuple(int(v) for v in r) for r in kinds['blocks']):
        assert (K, J) == (O.steps(n, sr), O.blocks(n, sr)), (sr, n)
        assert read == (K if J else 0)
        assert ws >= 8 * 8 * read // 8 * 5 + 2 * read          # states, segment sums, step sums, block means

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 24
    for name, code in answers.items():
        want = 0 if name.startswith('legal') else 2 if name.endswith('_above') else 1
        assert code == want, (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
