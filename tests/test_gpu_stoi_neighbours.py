"""tts_stoi beside MFMA GEMM launches of ANOTHER handle (another set of streams): the same bits as alone, in the manner of
tests/test_gpu_f0_neighbours.py -- an evaluation that measures intelligibility runs the stage on one batch while a second
engine may be busy on the same chip.  csrc/stoi.hip: double arithmetic, LDS, barriers and shuffles, no packed float32
arithmetic and no atomics."""
import numpy as np
import pytest

import stoi_cases as K
from neighbour_fixture import neighbour   # noqa: F401

pytestmark = pytest.mark.gpu


def test_stoi_beside_gemm_launches_of_another_handle(engine, neighbour):
    eng2, launch = neighbour
    keys = [('speech', 10), ('speech', 0), K.pattern_with_kept(94, seed=3), K.pattern_with_kept(36, gap_at=17, gap=6)] * 4
    rows = [K.row(k) for k in keys]
    lens = np.array([len(r[0]) for r in rows], np.int32)
    R, D = np.zeros((len(rows), int(lens.max())), np.float32), np.zeros((len(rows), int(lens.max())), np.float32)
    for b, (r, d) in enumerate(rows):
        R[b, :len(r)], D[b, :len(d)] = r, d
    d_r, d_d = engine.to_device(R), engine.to_device(D)
    try:
        run = lambda ext: engine.stoi(d_r, d_d, n_samples=lens, extended=ext, want_index=True, want_envelopes=True)
        quiet = {ext: run(ext) for ext in (False, True)}
        for ext in (False, True):       # ... and the quiet run is right
            for b in (0, 2):
                o = K.oracle(keys[b], ext)
                assert int(quiet[ext][0][b]['kept']) == o['kept'] and abs(float(quiet[ext][0][b]['value']) - o['value']) < 1e-9
        bad = n = 0
        for _ in range(6):
            launch()
            for ext in (False, True):
                got = run(ext)
                n += 1
                bad += not K.same_results(got, quiet[ext])
            eng2.synchronize()
        assert bad == 0, '%d of %d results differ from the quiet run' % (bad, n)
    finally:
        d_r.free()
        d_d.free()
