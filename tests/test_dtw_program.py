"""The host side of mel-cepstral distortion (csrc/dtw_plan.h: the cut of an anti-diagonal, the cells of a diagonal, the
direction-bit workspace and the argument checks of tts_dtw; csrc/cepstrum_plan.h: the DCT table and the checks of tts_mfcc) as a
stand-alone host program: tests/dtw_check.cpp with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the
host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and run.  What it prints is held
against the numpy oracles here: every integer exactly, table values to 4 ulp.  No GPU, nothing loaded into Python."""
import numpy as np

import cepstrum_oracle as C
import dtw_oracle as W
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_dtw_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('dtw_check.cpp', tmp_path)[0])
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

    # the refusal texts of the bad lengths, tts_mfcc's (n_frames) among them; a pair's n_a is looked at ahead of its n_b and
    # an earlier pair ahead of a later one
    want = {'n_a=%d' % n: LENGTH_REFUSAL.format(name='n_a', b=2, n=n, bound='Ta', hi=12) for n in (0, -1, 13)}
    want.update({'n_b=%d' % n: LENGTH_REFUSAL.format(name='n_b', b=0, n=n, bound='Tb', hi=20) for n in (0, -5, 21)})
    want.update({'n_frames=%d' % n: LENGTH_REFUSAL.format(name='n_frames', b=1, n=n, bound='T', hi=12) for n in (0, -1, 13)})
    want['order_pairs'] = LENGTH_REFUSAL.format(name='n_b', b=0, n=0, bound='Tb', hi=20)
    want['order_sides'] = LENGTH_REFUSAL.format(name='n_a', b=1, n=0, bound='Ta', hi=12)
    assert refusals == want
