"""The Griffin-Lim run planner (csrc/gl_plan.hip) as a stand-alone host program: tests/gl_plan_check.cpp with its own main,
compiled together with the planner as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes
(linked statically: the program needs nothing preloaded) -- and run over its grid of batches.  No GPU, nothing loaded into Python."""
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
    cmd += ['-x', 'c++', os.path.join(CSRC, 'gl_plan.hip'), os.path.join(ROOT, 'tests', 'gl_plan_check.cpp'), '-o', out]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_gl_plan_check_program(tmp_path):
    compilers = _compilers()
    assert compilers, 'no host C++ compiler (g++, c++, clang++, amdclang++ or $CXX)'
    exe = str(tmp_path / 'gl_plan_check')
    built = None
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
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode(errors='replace')
    print('built with', built[0], 'sanitizers' if built[1] else 'WITHOUT sanitizers')
    print(out[-3000:])
    assert run.returncode == 0, out[-3000:]
    assert ', 0 failures' in out
