"""The host side of STOI (csrc/stoi_plan.h: the frame and segment counts, the groupings and LDS bytes of the five launches, the
window, the band table and the argument checks of tts_stoi) as a stand-alone host program: tests/stoi_check.cpp with its own main,
compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically: the
program needs nothing preloaded) -- and run.  What it prints is held against tests/stoi_oracle.py here, every integer exactly.
No GPU, nothing loaded into Python."""
import numpy as np

import stoi_cases as K
import stoi_oracle as S
from host_checks import LENGTH_REFUSAL, build_and_run, length_refusals


def test_stoi_check_program(tmp_path):
    rows, refusals = length_refusals(build_and_run('stoi_check.cpp', tmp_path)[0])
    kinds = {k: [r[1:] for r in rows if r[0] == k] for k in ('consts', 'lds', 'frames', 'segments', 'scan', 'groups', 'band', 'window', 'check')}
    W, H, nfft, J, N, utts, energy_frames, scan_lanes, max_frames, group, env_lanes, seg_chunk, budget = (int(v) for v in kinds['consts'][0])
    assert (W, H, nfft, J, N) == (S.W, S.H, S.NFFT, S.J, S.N) and utts == 64
    assert (group, seg_chunk) == (K.GROUP, K.SEG_CHUNK) and max_frames == 65536 and budget <= 64 * 1024
    e_lds, env_lds, seg_lds = (int(v) for v in kinds['lds'][0])
    assert e_lds == 4 * (energy_frames + 1) * (H + 1) <= budget
    assert env_lds == 16 * (group * nfft + nfft // 2) + 8 * W <= budget          # 8 KB a frame, the twiddles, the window
    assert seg_lds == 8 * 2 * J * (seg_chunk + N - 1) <= budget

    assert len(kinds['frames']) == 13
    for n, F in kinds['frames']:
        assert int(F) == S.frames(int(n))
    assert dict((int(n), int(F)) for n, F in kinds['frames'])[255] == 0
    for kept, segs, length in kinds['segments']:
        assert int(segs) == S.segments(int(kept)) and int(length) == ((int(kept) - 1) * H + W if int(kept) else 0)
    for frames, run in kinds['scan']:
        assert int(run) == -(-int(frames) // scan_lanes)
    for count, per, g in kinds['groups']:
        assert int(g) == max(1, -(-int(count) // int(per)))

    w, bands = S.tables()
    assert [(int(a), int(b)) for _, a, b in kinds['band']] == [tuple(r) for r in bands.tolist()]
    assert np.array_equal(np.array([float(v) for _, v in kinds['window']]), w)

    answers = {name: int(code) for name, code in kinds['check']}
    assert len(answers) == 21
    for name, code in answers.items():
        want = 0 if name.startswith('legal') else 2 if name.endswith('_above') else 1
        assert code == want, (name, code)
    assert refusals == {'n_samples=%d' % n: LENGTH_REFUSAL.format(name='n_samples', b=1, n=n, bound='N', hi=5000) for n in (0, -1, 5001)}
