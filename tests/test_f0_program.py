"""The host side of F0 tracking (csrc/f0_plan.h: the frame count, the first sample of a frame, the frames a workgroup owns and its
LDS bytes, the lag bounds and the argument checks of tts_f0 and tts_f0_compare) as a stand-alone host program: tests/f0_check.cpp
with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked
statically: the program needs nothing preloaded) -- and run.  What it prints is held against tests/f0_oracle.py here, every
integer exactly.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT
import f0_oracle as Y

CSRC = os.path.join(ROOT, PKG, 'csrc')


def _compilers():
    names = [os.environ['CXX']] if os.environ.get('CXX') else []
    return [c for c in names + ['g++', 'c++', 'clang++', 'amdclang++'] if shutil.which(c)]


def _build(cxx, out, sanitize):
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-I', CSRC]
    if sanitize:
        cmd += ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer']
        if 'clang' not in subprocess.run([cxx, '--version'], stdout=subprocess.PIPE).stdout.decode():
            cmd += ['-static-libasan', '-static-libubsan']   # (clang links its sanitizer runtimes statically by default)
    cmd += [os.path.join(ROOT, 'tests', 'f0_check.cpp'), '-o', out]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_f0_check_program(tmp_path):
    compilers = _compilers()
    assert compilers, 'no host C++ compiler (g++, c++, clang++, amdclang++ or $CXX)'
    exe = str(tmp_path / 'f0_check')
    built, log = None, ''
    for sanitize in (True, False):   # without the flag only where no compiler can link the sanitizers' runtimes
        for cxx in compilers:
            r = _build(cxx, exe, sanitize)
            if r.returncode == 0:
                built = (cxx, sanitize)
                break
            log = r.stdout.decode(errors='replace')
        if built:
            break
    assert built, log[-3000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode(errors='replace')[-3000:]
    rows = [line.split() for line in run.stdout.decode().splitlines()]
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
    print('built with {} (sanitizers: {})'.format(*built))
