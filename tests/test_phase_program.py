"""The host side of the estimated initial phases (csrc/phase_plan.h: the cut of the frames into chunks and the argument checks of the estimate's entry
points) as a stand-alone host program: tests/phase_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer
and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  Its
chunk counts are held against the same arithmetic here.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT

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
    cmd += [os.path.join(ROOT, 'tests', 'phase_check.cpp'), '-o', out]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_phase_check_program(tmp_path):
    compilers = _compilers()
    assert compilers, 'no host C++ compiler (g++, c++, clang++, amdclang++ or $CXX)'
    exe = str(tmp_path / 'phase_check')
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
    chunk = int(rows[0][0])
    assert chunk >= 1 and len(rows) == 1 + 4 * chunk + 3
    for n, count in rows[1:]:
        assert int(count) == (0 if int(n) < 1 else -(-int(n) // chunk)), (n, count)
    print('built with {} (sanitizers: {})'.format(*built))
