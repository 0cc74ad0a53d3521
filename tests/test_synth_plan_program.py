"""The host-side plan of a synthesis call (csrc/synth_plan.h: the frame counts that end-of-speech stopping, the speaking rate and the
pitch leave a call, its refusals, and the per-utterance lengths) as a stand-alone host program: tests/synth_plan_check.cpp with its
own main, compiled as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes (linked statically:
the program needs nothing preloaded) -- and run.  Every row of its grid is held against the tests' own oracles here
(stretch_oracle, resample_oracle: numpy restatements of the reference's arithmetic), and the same grid against the two
functions of _hip.py that restate the plan for the Python callers.  No GPU, nothing loaded into Python."""
import numpy as np
import pytest

import resample_oracle as R
import stretch_oracle as S
from conftest import pkg
from host_checks import build_and_run

SIZES = [(2048, 275), (512, 100)]
FRAMES = range(4, 49)
RATES = [0.25, 0.8, 1.0, 1.2, 2.5, 4.0]
OCTAVES = [-1.0, -1.0 / 3.0, 0.0, 1.0 / 3.0, 1.0]
B = 3


def oracle_plan(n_fft, hop, T, s, octaves, stopping):
    """the plan from the oracles alone: an int -- which refusal, in the order a call meets them (2: the product outside [0.25, 4],
    3: rows shorter than min_frames with a pitch, 4: Griffin-Lim's frames, 5: stopping's) -- or a dict of what a legal call has"""
    minf = (n_fft // 2) // hop + 2            # the smallest n with hop (n - 1) > n_fft / 2
    assert hop * (minf - 1) > n_fft // 2 >= hop * (minf - 2)
    pitch, stretch = octaves != 0.0, s != 1.0 or octaves != 0.0
    rho = float(np.exp2(-np.float64(octaves)))
    eff = s * rho if pitch else s
    Tw = S.stretched_frames(T, s) if s != 1.0 else T
    Tg = T
    if stretch:
        if not S.RATE_MIN <= eff <= S.RATE_MAX:
            return 2
        if pitch and Tw < minf:
            return 3
        Tg = S.stretched_frames(T, eff)
        if Tg < minf:
            return 4
    if stopping and T < minf:
        return 5
    det = np.array([minf, (minf + T) // 2, T] if stopping else [T] * B, np.int32)
    gl = S.stretched_lengths(det, eff, Tg, minf) if stretch else det
    reported = gl if not pitch else (S.stretched_lengths(det, s, Tw, minf) if s != 1.0 else det)
    n_samples, keep = hop * (gl - 1), hop * (reported - 1)
    kept = [min(R.resampled_valid(int(n), rho), int(k)) if pitch else -1 for n, k in zip(n_samples, keep)]
    have = pitch and stopping
    total = int(gl.sum())
    return dict(stretch=stretch, pitch=pitch, rate=eff, rate_s=s, rho=rho if pitch else 1.0, Tw=Tw, Tg=Tg, min_frames=minf,
                ragged=total != B * Tg, T_model=-(-total // B), detected=det.tolist() if stopping else [-1] * B,
                reported=reported.tolist(), gl=gl.tolist(), n_samples=n_samples.tolist() if have else [-1] * B,
                keep=keep.tolist() if have else [-1] * B, kept=kept)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    return build_and_run('synth_plan_check.cpp', tmp_path_factory.mktemp('synth_plan'))[0]


def _grid():
    for n_fft, hop in SIZES:
        for T in FRAMES:
            for s in RATES:
                for o in OCTAVES:
                    for stopping in (False, True):
                        yield n_fft, hop, T, s, o, stopping


def test_the_program_agrees_with_the_oracles(rows):
    grid = list(_grid())
    assert len(rows) == len(grid) == 2 * 45 * 6 * 5 * 2
    legal = refused = 0
    for row, point in zip(rows, grid):
        n_fft, hop, T, s, o, stopping = point
        assert (int(row[0]), int(row[1]), int(row[2]), float(row[3]), float(row[4]), int(row[5])) == (n_fft, hop, T, s, o, int(stopping))
        want = oracle_plan(*point)
        if isinstance(want, int):        # an illegal row must be refused, and by the refusal a call meets first
            assert row[6:] == ['R', str(want)], (point, row)
            refused += 1
            continue
        assert row[6] == 'OK', (point, row)          # a row the oracle calls legal must not be refused
        legal += 1
        got = dict(stretch=bool(int(row[7])), pitch=bool(int(row[8])), rate=float(row[9]), rate_s=float(row[10]), rho=float(row[11]),
                   Tw=int(row[12]), Tg=int(row[13]), min_frames=int(row[14]), ragged=bool(int(row[15])), T_model=int(row[16]))
        per = np.array([int(v) for v in row[17:]], np.int64).reshape(B, 6)
        for i, name in enumerate(('detected', 'reported', 'gl', 'n_samples', 'keep', 'kept')):
            got[name] = per[:, i].tolist()
        assert got == want, (point, got, want)
        if not want['stretch']:          # rate 1.0 and pitch 0: nothing of the call changes
            assert want['Tw'] == want['Tg'] == T and want['gl'] == want['reported'] == ([T] * B if not stopping else want['detected'])
    print('{} legal rows, {} refused'.format(legal, refused))
    assert legal > 3000 and refused > 500


def test_the_python_plan_is_the_same_plan():
    """_hip.synth_frame_counts / synth_lengths over the same grid: the C++ copy and the Python copy cannot drift apart"""
    H = pkg('_hip')
    for point in _grid():
        n_fft, hop, T, s, o, stopping = point
        want = oracle_plan(*point)
        if want == 2:
            with pytest.raises(ValueError):
                H.synth_frame_counts(T, s, o)
            continue
        counts = H.synth_frame_counts(T, s, o)
        if isinstance(want, int):        # too short for Griffin-Lim: the callers' refusal, made from these counts
            minf = (n_fft // 2) // hop + 2
            assert min(counts) < minf or (stopping and T < minf), point
            continue
        assert counts == (want['Tw'], want['Tg']) and H.pitch_frames(T, s, o) == want['Tg'], point
        det = want['detected'] if stopping else [T] * B
        reported, gl = H.synth_lengths(det, T, s, o, want['min_frames'])
        assert reported.dtype == gl.dtype == np.int32
        assert (reported.tolist(), gl.tolist()) == (want['reported'], want['gl']), point
