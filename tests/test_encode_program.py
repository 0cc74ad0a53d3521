"""The host side of the delivery encoder (csrc/encode_plan.h: the per-sample function, the G.711 segment search, the dither, the
tile arithmetic and the argument checks of tts_encode and tts_set_output) as a stand-alone host program: tests/encode_check.cpp
with its own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked
statically: the program needs nothing preloaded) -- and run.  What it prints is held against tests/encode_oracle.py here.  No GPU,
nothing loaded into Python."""
import numpy as np

import encode_cases as C
import encode_oracle as O
from host_checks import build_and_run, length_refusals


def _checksum(codes):
    s = 0
    for c in codes.tolist():
        s = (s * 1000003 + c) & (2 ** 64 - 1)
    return s


def test_encode_check_program(tmp_path):
    rows, msgs = length_refusals(build_and_run('encode_check.cpp', tmp_path)[0])
    kinds = {}
    for r in rows:
        kinds.setdefault(r[0], []).append(r[1:])
    utts, lanes, group, tile = (int(v) for v in kinds['consts'][0])
    assert group == 4 and tile % (lanes * group) == 0 and utts >= 1 and lanes % 64 == 0
    assert [(int(f), int(w)) for f, w in kinds['width']] == [(-1, -1), (0, 4), (1, 2), (2, 1), (3, 1), (4, 1), (5, -1)]
    assert [tuple(int(v) for v in r) for r in kinds['silence']] == [(f, O.SILENCE[f], O.SILENCE[f]) for f in O.FORMATS]

    # every level x 4 formats: the oracle's codes (int16 as its 16 bits), the records
    x = C.all_levels()
    for f, marked, summed in zip(O.FORMATS, kinds['levels'], kinds['levelsum']):
        codes, st = O.encode(x[None], f)
        codes = codes[0].astype(np.int64) & 0xFFFF
        assert int(marked[0]) == f and [int(v) for v in marked[1:]] == codes[::257].tolist(), f
        assert [int(v) for v in summed] == [f, _checksum(codes), int(st['clipped'][0]), int(st['nans'][0]), int(st['peak'][0])], f

    xs, q16, clipped, nans, peak = C.specials()
    for Q, fmt, got, count in zip((32768, 128), (O.S16, O.U8), kinds['special'], kinds['specialcount']):
        q, cl, na = O.quantise(xs, fmt)
        assert int(got[0]) == Q and [int(v) for v in got[1:]] == q.tolist(), Q
        assert [int(v) for v in count] == [Q, int(cl.sum()), int(na.sum()), int(np.abs(q).max())], Q
    assert [int(v) for v in kinds['special'][0][1:]] == q16.tolist() and [int(v) for v in kinds['specialcount'][0][1:]] == [clipped, nans, peak]

    assert len(kinds['dither']) == 45
    for seed, b, i, d in kinds['dither']:
        assert float(d) == O.dither(int(seed), int(b), np.array([int(i)]))[0], (seed, b, i)
    want = O.encode_row(0.25 * C.LSB * np.arange(16, dtype=np.float32), O.S16, O.TPDF, 1234, b=2)[0]
    assert [int(v) for v in kinds['dithered'][0]] == (want.astype(np.int64) & 0xFFFF).tolist()

    assert [tuple(int(v) for v in r) for r in kinds['tiles']] == [(1, 1), (tile - 1, 1), (tile, 1), (tile + 1, 2), (2 ** 31 - 1, -(-(2 ** 31 - 1) // tile))]
    assert [tuple(int(v) for v in r) for r in kinds['head']] == [(e, -e % 4) for e in range(8)]

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 15
    for name, code in answers.items():
        assert code == (0 if name.startswith('legal') else 1), (name, code)
    assert msgs['n_samples=-1'] == 'n_samples[1] = -1 is not in 0 .. N = 5000' and msgs['n_samples=5001'] == 'n_samples[1] = 5001 is not in 0 .. N = 5000'
    assert 'TTS_FMT_F32' in msgs['f32']

    outputs = {name: (int(code), int(on)) for name, code, on in kinds['output']}
    assert len(outputs) == 13
    on = {'legal_off': 0, 'legal_off_no_rates': 0}
    for name, (code, is_on) in outputs.items():
        if name.startswith('legal'):
            assert (code, is_on) == (0, on.get(name, 1)), name
        else:
            assert (code, is_on) == (1, 1), name   # (refused: *on keeps what it held)
