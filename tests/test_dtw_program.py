"""The host side of mel-cepstral distortion (csrc/dtw_plan.h: the cut of an anti-diagonal, the cells of a diagonal, the
direction-bit workspace and the argument checks of tts_dtw; csrc/cepstrum_plan.h: the DCT table and the checks of tts_mfcc) as a
stand-alone host program: tests/dtw_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the
host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held
against the numpy oracles here: every integer exactly, table values to 4 ulp.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np

from conftest import PKG, ROOT
import cepstrum_oracle as C
import dtw_oracle as W

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
    cmd += [os.path.join(ROOT, 'tests', 'dtw_check.cpp'), '-o', out]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def test_dtw_check_program(tmp_path):
    compilers = _compilers()
    assert compilers, 'no host C++ compiler (g++, c++, clang++, amdclang++ or $CXX)'
    exe = str(tmp_path / 'dtw_check')
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
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'shape', 'diag', 'slots', 'dir', 'dtw_check', 'tab')}
    tile, slots, max_frames, max_d, pairs, dir_cells = (int(v) for v in kinds['consts'][0])
    assert max_frames >= 2048 and max_frames == tile * slots and max_d == 128 and dir_cells == 16 and pairs >= 1

    # the grid: 1 x 1, 1 x n, n x 1 and the cut from both sides
    sizes = [1, 2, 9, tile - 1, tile, tile + 1]
    assert [(int(a), int(b)) for a, b, _, _ in kinds['shape']] == [(a, b) for a in sizes for b in sizes]
    for na, nb, nd, sl in kinds['shape']:
        assert int(nd) == int(na) + int(nb) - 1 and int(sl) == -(-int(na) // tile)
    assert len(kinds['diag']) == sum(a + b + 1 for a in sizes for b in sizes)
    for na, nb, k, lo, hi in kinds['diag']:
        na, nb, k = int(na), int(nb), int(k)
        if 0 <= k <= na + nb - 2:
            assert (int(lo), int(hi)) == W.diag_range(k, na, nb), (na, nb, k)
        else:
            assert int(lo) > int(hi), (na, nb, k)
    for na, sl in kinds['slots']:
        assert int(sl) == -(-int(na) // tile)
    assert len(kinds['dir']) == 3 * 4 * 6
    for B, r, c, words, pair, nbytes in kinds['dir']:
        B, r, c = int(B), int(r), int(c)
        assert int(words) == -(-c // 16) and int(pair) == r * int(words) and int(nbytes) == 4 * B * int(pair)
        assert 8 * int(nbytes) >= 2 * B * r * c   # 2 bits per cell

    answers = {name: int(code) for name, code in kinds['dtw_check']}
    assert len(answers) == 22
    for name, code in answers.items():
        want = 0 if name.startswith('legal') else 2 if name.endswith('_above') else 1
        assert code == want, (name, code)

    # the DCT table against the oracle's own: each entry is a few roundings and one cos away
    mats = {}
    assert len(kinds['tab']) >= 100
    for n_mels, n_mfcc, n, k, v in kinds['tab']:
        key = (int(n_mels), int(n_mfcc))
        if key not in mats:
            mats[key] = C.dct_matrix(*key)
        want = mats[key][int(k), int(n)]
        assert abs(float(v) - want) <= 4 * np.spacing(abs(want)) + 1e-300, (key, n, k, v, want)
    print('built with {} (sanitizers: {})'.format(*built))
