"""The host side of the watermark (csrc/watermark_plan.h: the constants, the workspace sizes, the hash, the carrier, the block
envelope, the marked sample, v, the chip sums, and the argument checks of tts_watermark_embed, tts_watermark_detect and
tts_set_watermark) as a stand-alone host program: tests/watermark_check.cpp with its own main, compiled as plain C++ -- with
AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the program needs nothing preloaded) -- and
run.  What it prints is held against tests/watermark_oracle.py here: every integer exactly, every float bit for bit (they travel as
hex floats).  No GPU, nothing loaded into Python."""
import numpy as np

import watermark_cases as C
import watermark_oracle as O
from host_checks import build_and_run, length_refusals

KNOWN = O.Params(0x0123456789ABCDEF, 0xB6, 8, 6, 5, 0.03125)


def sample(i):
    return np.float32(np.float32(((i * 37) % 101 - 50) / 64.0) * np.float32(1.0 if i % 700 < 350 else 0.03125))


def test_watermark_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('watermark_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'ws', 'lds', 'hash', 'carrier', 'row', 'chip', 'refuse', 'check')}
    c = kinds['consts'][0]
    assert [int(v) for v in c[:5]] == [O.BLOCK, O.BITS_MAX, O.CHIP_MIN, O.CHIP_MAX, O.SYMBOL_MAX] == [64, 32, 2, 16, 65536]
    assert float.fromhex(c[5]) == O.STRENGTH_MAX == 0.25
    assert [int(v) for v in c[6:]] == [O.MAX_OFFSETS, O.UTTS, O.TILE, O.CORR_TILE, O.CORR_THREADS, O.V_MAX] == [4096, 64, 4096, 2048, 128, 127]
    assert len(kinds['ws']) == 8 * 3 * 5
    for r in kinds['ws']:
        n, L, D = (int(v) for v in r[:3])
        want = (O.blocks(n), O.tiles(n), O.chips(n, L), O.corr_tiles(n, L), O.corr_tiles(n, L) * O.CORR_TILE, O.shifts(D, L), O.corr_shifts(D, L),
                O.corr_ranges(D, L), O.sign_words(n, L, D))
        assert tuple(int(v) for v in r[3:]) == want, (n, L, D)
        # what the kernels rest on: a workgroup's shifts times its sub-ranges are its threads, every shift lies in a range, and the
        # signs cover every chip a shifted tile reads
        sw, ranges = want[6], want[7]
        assert O.CORR_THREADS % sw == 0 and sw * ranges >= want[5] and want[8] * 32 >= want[4] + sw * ranges + 64
        assert want[4] >= want[2] and want[4] % 2 == 0
    assert [tuple(int(v) for v in r[3:]) for r in kinds['ws'][:2]] == [(1, 1, 1, 1, 2048, 1, 1, 1, 67), (1, 1, 1, 1, 2048, 5, 8, 1, 67)]
    assert [tuple(int(v) for v in r) for r in kinds['lds']] == [(P, O.corr_lds(P)) for P in (1, 16, 32)]

    assert len(kinds['hash']) == 20
    for key, q, z, neg in kinds['hash']:
        assert int(z) == int(O.hash64(int(key), np.array([int(q)], np.uint64))[0]), (key, q)
        assert 1 - 2 * int(neg) == int(O.chip_sign(int(key), np.array([int(q)], np.uint64))[0])
    pos = np.array([int(r[0]) for r in kinds['carrier']])
    assert len(pos) == 701 and pos[-1] == 2 ** 40 + 12345
    got = np.array([int(r[1]) for r in kinds['carrier']])
    assert np.array_equal(got, O.carrier(KNOWN, pos)) and set(got.tolist()) == {-1, 1}

    # the row: the envelope, the marked samples and v
    x = np.array([sample(i) for i in range(700)], np.float32)
    x[100], x[101], x[102], x[300] = np.nan, np.inf, -0.0, np.float32(1e-45)
    e = np.array([float.fromhex(r[1]) for r in kinds['row']], np.float32)
    y = np.array([float.fromhex(r[2]) for r in kinds['row']], np.float64).astype(np.float32)
    m = np.array([int(r[3]) for r in kinds['row']], bool)
    v = np.array([int(r[4]) for r in kinds['row']])
    assert np.array_equal(C.bits(e), C.bits(O.envelope(x)))
    want, marked = O.embed(x, KNOWN)
    assert C.same(y, want) and np.array_equal(m, marked) and marked.sum() > 400 and not marked[:64].any() and not marked[640:].any()
    assert np.array_equal(v, O.v_of(x)) and v.max() == 127 and v.min() == -127 and (v == 0).sum() > 100
    for L in (2, 6, 16):
        for f in range(L):
            got = np.array([int(r[3]) for r in kinds['chip'] if int(r[0]) == L and int(r[1]) == f])
            assert np.array_equal(got, O.chip_sums(v, L, f)), (L, f)

    answers = {name: int(code) for name, code in kinds['refuse']}
    assert len(answers) == 14
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), name
    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 17 + 16
    for name, code in answers.items():
        assert code == (0 if 'legal' in name else 1), (name, code)
    assert refusals == {'n_samples=%d' % n: 'n_samples[1] = %d is not in 0 .. N = 5000' % n for n in (-1, 5001)}
