"""What the host-only tests share: building and running a stand-alone check program (tests/*_check.cpp, plain C++ with its own
main) and an Engine object that never reaches the library.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT, pkg

CSRC = os.path.join(ROOT, PKG, 'csrc')


def _compilers():
    names = [os.environ['CXX']] if os.environ.get('CXX') else []
    return [c for c in names + ['g++', 'c++', 'clang++', 'amdclang++'] if shutil.which(c)]


def _build(cxx, sources, out, sanitize):
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-I', CSRC]
    if sanitize:
        cmd += ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer']
        if 'clang' not in subprocess.run([cxx, '--version'], stdout=subprocess.PIPE).stdout.decode():
            cmd += ['-static-libasan', '-static-libubsan']   # (clang links its sanitizer runtimes statically by default)
    return subprocess.run(cmd + sources + ['-o', out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def build_and_run(source_name, tmp_path, with_csrc=(), timeout=120):
    """Compiles tests/``source_name`` (and the files ``with_csrc`` of csrc/, as C++) with AddressSanitizer and UBSan linked
    statically -- without them only where no compiler can link their runtimes -- runs the program and returns ``(rows, built)``:
    its output lines split at blanks, and ``(compiler, sanitizers)``."""
    compilers = _compilers()
    assert compilers, 'no host C++ compiler (g++, c++, clang++, amdclang++ or $CXX)'
    exe = str(tmp_path / os.path.splitext(source_name)[0])
    sources = [a for f in with_csrc for a in ('-x', 'c++', os.path.join(CSRC, f))] + [os.path.join(ROOT, 'tests', source_name)]
    built, log = None, ''
    for sanitize in (True, False):
        for cxx in compilers:
            r = _build(cxx, sources, exe, sanitize)
            if r.returncode == 0:
                built = (cxx, sanitize)
                break
            log = r.stdout.decode(errors='replace')
        if built:
            break
    assert built, log[-3000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert run.returncode == 0, (run.stdout + run.stderr).decode(errors='replace')[-3000:]
    print('built with {} (sanitizers: {})'.format(*built))
    return [line.split() for line in run.stdout.decode().splitlines()], built


LENGTH_REFUSAL = '{name}[{b}] = {n} is not in 1 .. {bound} = {hi}'   # what every stage answers to a length outside its buffer


def length_refusals(rows):
    """``(the other rows, {case: refusal text})`` of a program that prints its bad-length cases as ``msg <case> <text>``"""
    return [r for r in rows if r[0] != 'msg'], {r[1]: ' '.join(r[2:]) for r in rows if r[0] == 'msg'}


def no_device_engine():
    """an Engine object that was never given a handle: every call on it must raise before it reaches the library"""
    H = pkg('_hip')
    eng = H.Engine.__new__(H.Engine)
    eng.handle = None
    eng.lib = None
    eng._init_settings()
    return eng
