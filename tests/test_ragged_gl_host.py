"""CPU: the host side of the ragged Griffin-Lim call (tts_griffin_lim_ragged) -- the cut of a ragged batch into runs
(tts_debug_gl_plan_ragged), the fairness of the bounds test_gpu_ragged_gl.py holds the kernels to, and the Python surface
(``n_frames`` of audio.synthesis, datasets.statistics.collect_reconstruction_error, the two command-line flags) against
stand-in engines.  Reference: audio/synthesis.py:43-125 (griffin_lim_v2), datasets/statistics.py:146-187."""
import ctypes
import heapq
import os

import numpy as np
import pytest

import audio_cases as C
import ragged_cases as R
from conftest import pkg
from parity import assert_segment_parity

WIN, HOP = 1102, 275
RUN_COST = 11        # what a run costs beyond its frames, in frames (gl_plan_items: "Sum T_b + 11 per run")
MIN_RUN = 8          # the shortest run the dealer cuts: one round of the eight waves

LENGTH_VECTORS = {'short': [5, 8, 9, 23, 40], 'one-long': [1000] + [5] * 63,
                  'spread': [int(round(x)) for x in np.linspace(300, 1000, 64)]}


def _items(buf, n):
    return [(buf[4 * k], buf[4 * k + 1], buf[4 * k + 2], buf[4 * k + 3]) for k in range(n)]


def plan_ragged(lengths, workers, win=WIN, hop=HOP):
    lib = pkg('_hip').load_library()
    cap = 16384
    buf = (ctypes.c_int * (4 * cap))()
    ring = ctypes.c_int(0)
    a = np.ascontiguousarray(lengths, dtype=np.int32)
    n = lib.tts_debug_gl_plan_ragged(a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(lengths), win, hop, workers, buf, cap,
                                     ctypes.byref(ring))
    assert 1 <= n <= cap, n
    return _items(buf, n), ring.value


def plan_uniform(T, B, workers, win=WIN, hop=HOP):
    lib = pkg('_hip').load_library()
    cap = 16384
    buf = (ctypes.c_int * (4 * cap))()
    ring = ctypes.c_int(0)
    n = lib.tts_debug_gl_plan(T, B, win, hop, workers, buf, cap, ctypes.byref(ring))
    assert 1 <= n <= cap, n
    return _items(buf, n), ring.value


def schedule(items, workers):
    """(costliest worker, mean) of the list schedule the kernel's item counter produces: the table in order, every entry to
    the worker that comes free first; a run costs its frames + RUN_COST"""
    heap = [(0, k) for k in range(workers)]
    heapq.heapify(heap)
    for _, _, n, _ in items:
        load, k = heapq.heappop(heap)
        heapq.heappush(heap, (load + n + RUN_COST, k))
    loads = [l for l, _ in heap]
    return max(loads), sum(loads) / float(workers)


@pytest.mark.parametrize('workers', [16, 192, 256])
@pytest.mark.parametrize('name', sorted(LENGTH_VECTORS))
def test_ragged_plan_covers_every_frame_once_and_balances_like_the_uniform_one(name, workers):
    """Every frame of every utterance lies in exactly one run, no run leaves its utterance, the slot words are those of the
    uniform plan (a run's ordinal in its utterance; the last run carries the slots other utterances have beyond it), and
    the costliest worker is as close to the mean as the uniform batch of the same B and sum of frames is on the same
    workers -- that ratio is taken from tts_debug_gl_plan here, not from a constant.  One allowance on top, from what a
    ragged batch cannot avoid and a uniform one of whole utterances per worker can: a share ends at an utterance's end or
    at least MIN_RUN frames from it, and may hold one run more than the mean share -- RUN_COST + MIN_RUN frames."""
    lengths = LENGTH_VECTORS[name]
    B = len(lengths)
    items, ring = plan_ragged(lengths, workers)
    assert ring >= 8
    runs = {}
    for b, t0, n, w in items:
        assert 0 <= b < B and n >= 1 and t0 >= 0 and t0 + n <= lengths[b], (b, t0, n)
        runs.setdefault(b, []).append((t0, n, w))
    assert sorted(runs) == list(range(B))
    spu = max(len(r) for r in runs.values())
    for b, r in runs.items():
        r.sort()
        t = 0
        for k, (t0, n, w) in enumerate(r):
            assert t0 == t, (b, r)
            t += n
            assert (w & 0xffff) == k
            assert (w >> 16) == (spu - len(r) if k == len(r) - 1 else 0)
        assert t == lengths[b]
    assert plan_ragged(lengths, workers)[0] == items   # same inputs, same cut
    total = sum(lengths)
    uniform, _ = plan_uniform(-(-total // B), B, workers)
    worst_u, mean_u = schedule(uniform, workers)
    worst, mean = schedule(items, workers)
    print('{} on {}: ragged {} runs, worst {} mean {:.1f} ({:.3f}); uniform {} runs, worst {} mean {:.1f} ({:.3f})'.format(
        name, workers, len(items), worst, mean, worst / mean, len(uniform), worst_u, mean_u, worst_u / mean_u))
    assert worst <= worst_u / mean_u * mean + RUN_COST + MIN_RUN


@pytest.mark.parametrize('T,B,workers,win,hop', [(40, 5, 16, 1102, 275), (1000, 64, 256, 1102, 275), (333, 7, 192, 800, 200),
                                                 (5, 64, 16, 1102, 275), (813, 5, 224, 1102, 275)])
def test_uniform_lengths_give_the_uniform_plan_item_for_item(T, B, workers, win, hop):
    assert plan_ragged([T] * B, workers, win, hop) == plan_uniform(T, B, workers, win, hop)


def test_plan_entry_point_refusals():
    lib = pkg('_hip').load_library()
    buf = (ctypes.c_int * 64)()
    a = np.array([5, 0, 9], np.int32)
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.tts_debug_gl_plan_ragged(p, 3, WIN, HOP, 16, buf, 16, None) < 0       # a length of 0
    assert lib.tts_debug_gl_plan_ragged(None, 3, WIN, HOP, 16, buf, 16, None) < 0
    a[1] = 8
    assert lib.tts_debug_gl_plan_ragged(p, 3, WIN, HOP, 0, buf, 16, None) < 0        # no workers
    assert lib.tts_debug_gl_plan_ragged(p, 3, WIN, HOP, 16, buf, 16, None) >= 3


# ---------------------------------------------------------------------------------------------- float32 margin
@pytest.mark.parametrize('k', range(len(R.HOST_TABLE)))
def test_float32_restatement_keeps_a_quarter_of_the_bounds_on_the_gpu_tests_inputs(k):
    """audio_cases.griffin_lim32 on every utterance the GPU tests feed the kernels, against the float64 oracle: within
    HOST_MARGIN of gl_tol(n_iter) per hop segment and of 1e-3 relative on the mse"""
    cfg, lengths, n_iter = R.HOST_TABLE[k]
    n_fft, win, hop = cfg
    for T in lengths:
        mag, init = R.utterance(cfg, T)
        ref_wav, ref_mse = R.reference(cfg, T, n_iter)
        wav, mse = C.griffin_lim32(mag, win, hop, n_fft, n_iter, init)
        assert_segment_parity(wav, ref_wav, hop, C.HOST_MARGIN * C.gl_tol(n_iter), 'f32 {} T={} it={}'.format(cfg, T, n_iter))
        print('f32 {} T={}: mse {} vs {}'.format(cfg, T, mse, ref_mse))
        assert abs(mse - ref_mse) <= C.HOST_MARGIN * 1e-3 * abs(ref_mse) + 1e-9


def test_every_gpu_case_is_in_the_host_table():
    table = {(cfg, T, n) for cfg, lengths, n in R.HOST_TABLE for T in lengths}
    for cfg, lengths, n_iter in [(R.STREAM, R.STREAM_LENGTHS, 4), (R.STREAM, R.STREAM_LENGTHS[:1] + R.STREAM_LENGTHS[2:3], 1),
                                 (R.STREAM_800, R.STREAM_800_LENGTHS, 4), (R.GENERAL_1024, R.GENERAL_1024_LENGTHS, 3),
                                 (R.GENERAL_512, R.GENERAL_512_LENGTHS, 3)]:
        for T in lengths:
            assert (cfg, T, n_iter) in table


def test_an_utterance_is_the_same_array_in_every_batch():
    mag, init = R.batch(R.STREAM, [5, 9])
    mag2, init2 = R.batch(R.STREAM, [9, 23, 5], fill=np.nan)
    assert np.array_equal(mag[1], mag2[0, :, :9]) and np.array_equal(init[0, :, :5], init2[2, :, :5])
    assert np.isnan(mag2[0, :, 9:]).all() and np.isnan(init2[2, :, 5:]).all() and not np.isnan(mag2[1]).any()
    assert (mag[0, :, 5:] == 0).all()


# ---------------------------------------------------------------------------------------------- the Python surface
class _NoEngine(object):
    """stands where an Engine would: any use of it is the failure"""

    def __getattr__(self, name):
        raise AssertionError('the engine was touched ({})'.format(name))


class _Dev(object):
    def __init__(self, a):
        self.a = np.asarray(a)

    def to_host(self):
        return self.a


class _FakeEngine(object):
    """Records the calls; stft_magnitude gives every recording a spectrogram that names it (its first sample in every bin,
    its frame index added), griffin_lim a waveform and an mse that name the utterance's length."""

    def __init__(self):
        self.stft_calls, self.gl_calls = [], []

    def stft_magnitude(self, wav, n_fft, win, hop, power=1.0):
        wav = np.asarray(wav)
        self.stft_calls.append((wav.shape, n_fft, win, hop))
        Tf = 1 + wav.shape[1] // hop
        return _Dev(wav[:, :1, None] + np.zeros((1, 1 + n_fft // 2, 1), np.float32) + np.arange(Tf, dtype=np.float32)[None, None, :])

    def griffin_lim(self, mag, n_iter, win, hop, n_fft, init_phase=None, seed=0, want_mse=True, momentum=None, n_frames=None):
        mag = np.asarray(mag)
        self.gl_calls.append(dict(mag=mag.copy(), n_iter=n_iter, win=win, hop=hop, n_fft=n_fft, seed=seed, momentum=momentum,
                                  init=None if init_phase is None else np.asarray(init_phase).copy(),
                                  n_frames=None if n_frames is None else [int(n) for n in n_frames]))
        B, _, T = mag.shape
        nf = [T] * B if n_frames is None else list(n_frames)
        wav = np.zeros((B, hop * (T - 1)), np.float32)
        for b, n in enumerate(nf):
            wav[b, :hop * (n - 1)] = n
        return _Dev(wav), _Dev(np.array([mag[b, 0, 0] + 1000.0 * nf[b] for b in range(B)], np.float32))


def test_griffin_lim_v2_with_n_frames_returns_per_utterance_arrays():
    S = pkg('audio.synthesis')
    eng = _FakeEngine()
    mag = np.ones((3, 1025, 40), np.float32)
    wavs, mse = S.griffin_lim_v2(mag, 1102, 275, 2048, 2, seed=3, engine=eng, n_frames=[5, 40, 23])
    assert [w.shape for w in wavs] == [(275 * 4,), (275 * 39,), (275 * 22,)]
    assert [float(w[0]) for w in wavs] == [5, 40, 23] and mse.shape == (3,)
    call = eng.gl_calls[0]
    assert call['n_frames'] == [5, 40, 23] and call['seed'] == 3 and call['momentum'] == 0.0
    out = S.spectrogram_to_wav(mag, 1102, 275, 2048, 2, seed=3, engine=eng, n_frames=np.array([5, 40, 23]))
    assert isinstance(out, list) and [w.dtype for w in out] == [np.float32] * 3 and len(out[2]) == 275 * 22
    wavs0, mse0 = S.griffin_lim_v2(mag, 1102, 275, 2048, 0, seed=3, engine=eng, n_frames=[5, 40, 23])
    assert mse0 is None and len(wavs0) == 3
    # without n_frames nothing changes: one array, no n_frames passed on
    wav, _ = S.griffin_lim_v2(mag, 1102, 275, 2048, 2, seed=3, engine=eng)
    assert wav.shape == (3, 275 * 39) and eng.gl_calls[-1]['n_frames'] is None


@pytest.mark.parametrize('n_frames', [[5, 0, 9], [5, 41, 9], [5, 4, 9], [5, 9], [[5, 9, 9]] * 2])
def test_n_frames_refusals_come_before_the_engine(n_frames):
    """a length of 0, one above T_max, one too short for the reflect padding (275 * 3 <= 1024), a wrong count"""
    S = pkg('audio.synthesis')
    mag = np.ones((3, 1025, 40), np.float32)
    with pytest.raises(ValueError):
        S.griffin_lim_v2(mag, 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), n_frames=n_frames)
    with pytest.raises(ValueError):
        S.spectrogram_to_wav(mag, 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), n_frames=n_frames)


def test_n_frames_needs_a_batch_and_a_momentum_in_range():
    S = pkg('audio.synthesis')
    with pytest.raises(ValueError):
        S.griffin_lim_v2(np.ones((1025, 40), np.float32), 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), n_frames=[40])
    for momentum in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError):
            S.griffin_lim_v2(np.ones((2, 1025, 40), np.float32), 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), n_frames=[40, 9],
                             momentum=momentum)
    H = pkg('_hip')
    assert H.ragged_frame_counts([5, 40], 2, 40, 275, 2048).dtype == np.int32
    with pytest.raises(ValueError, match=r'n_frames\[1\]'):
        H.ragged_frame_counts([5, 4], 2, 40, 275, 2048)


def _write_wavs(tmp_path, specs):
    """specs: (name, samples, sampling rate); the first sample names the file"""
    io = pkg('audio.io')
    paths = []
    for k, (name, n, sr) in enumerate(specs):
        w = np.zeros(n, np.float32)
        w[0] = 0.01 * (k + 1)
        p = str(tmp_path / name)
        io._write_float32_wav(p, w, sr)
        paths.append(p)
    return paths


def test_collect_reconstruction_error_batches_by_rate_and_length(tmp_path, capsys):
    """Batches of `batch_size` files; inside a batch one ragged call per sampling rate, its recordings sorted by length,
    n_fft 2048 with 50 ms / 12.5 ms through ms_to_samples; the result is the mean of the per-file mse, printed under the
    reference's words; bytes paths are accepted."""
    ST = pkg('datasets.statistics')
    specs = [('a.wav', 9000, 22050), ('b.wav', 3000, 16000), ('c.wav', 4000, 22050), ('d.wav', 7000, 22050), ('e.wav', 5000, 16000)]
    paths = _write_wavs(tmp_path, specs)
    eng = _FakeEngine()
    listing = [p.encode() if k % 2 else p for k, p in enumerate(paths)]
    init = {p: None for p in paths}
    frames_of = {}
    for p, (_, n, sr) in zip(paths, specs):
        hop = int(12.5 / 1000 * sr)
        frames_of[p] = 1 + n // hop
        init[p] = np.full((1025, frames_of[p]), 0.25, np.float32)
    total = ST.collect_reconstruction_error(listing, 7, batch_size=4, seed=11, engine=eng, init_phases=init)
    out = capsys.readouterr().out
    assert 'Collecting reconstruction statistics for 5 files ...' in out
    assert 'Dataset MSE with 7 iterations: {}'.format(total) in out
    # batch 1 = a b c d: 16 kHz (b) and 22.05 kHz (c, d, a by length); batch 2 = e
    calls = eng.gl_calls
    assert [(c['win'], c['hop'], c['n_fft'], c['n_iter']) for c in calls] == [(800, 200, 2048, 7), (1102, 275, 2048, 7), (800, 200, 2048, 7)]
    assert calls[0]['n_frames'] == [frames_of[paths[1]]]
    assert calls[1]['n_frames'] == [frames_of[paths[2]], frames_of[paths[3]], frames_of[paths[0]]]
    assert calls[2]['n_frames'] == [frames_of[paths[4]]]
    m = calls[1]['mag']
    assert m.shape == (3, 1025, frames_of[paths[0]])
    assert [round(float(m[r, 0, 0]), 4) for r in range(3)] == [0.03, 0.04, 0.01]          # c, d, a: sorted by length
    assert (m[0, :, frames_of[paths[2]]:] == 0).all() and m[0, 5, 3] == np.float32(0.03) + 3  # zero padding behind its frames
    assert (calls[1]['init'][0, :, :frames_of[paths[2]]] == 0.25).all() and (calls[1]['init'][0, :, frames_of[paths[2]]:] == 0).all()
    assert calls[0]['momentum'] == 0.0 and calls[0]['seed'] == 11 and calls[2]['seed'] == 15   # seed + first index of the batch
    # recordings of one length share an analysis call; every other length has its own
    assert sorted(s[0] for s in eng.stft_calls) == sorted([(1, 3000), (1, 4000), (1, 7000), (1, 9000), (1, 5000)])
    expect = np.mean([0.01 * (k + 1) + 1000.0 * frames_of[p] for k, p in enumerate(paths)])
    assert total == pytest.approx(expect, rel=1e-6)


def test_dataset_statistics_flag(tmp_path, monkeypatch, capsys):
    """--reconstruction-iters N runs the statistic behind the dB constants; without the flag the output is what it was"""
    DS = pkg('tacotron.dataset_statistics')
    root = tmp_path / 'data'
    os.makedirs(str(root / 'wavs'))
    with open(str(root / 'metadata.csv'), 'w') as f:
        f.write('x1|A CAT|a cat\n')
    seen = []
    monkeypatch.setattr(DS, 'collect_decibel_statistics', lambda paths: (1.0, 2.0, 3.0, 4.0))
    monkeypatch.setattr(DS, 'collect_reconstruction_error', lambda paths, n: seen.append((list(paths), n)) or 0.5)
    assert DS.main(['--dataset-folder', str(root)]) == 0
    plain = capsys.readouterr().out
    assert seen == [] and plain.rstrip().endswith('linear_mag_max_db =  1.0')
    assert DS.main(['--dataset-folder', str(root), '--reconstruction-iters', '60']) == 0
    assert capsys.readouterr().out.startswith(plain.rstrip('\n')) and len(seen) == 1 and seen[0][1] == 60 and len(seen[0][0]) == 1
    with pytest.raises(SystemExit):
        DS.main(['--dataset-folder', str(root), '--reconstruction-iters', '0'])


def test_gta_wav_flag_needs_wav_for_its_iterations():
    G = pkg('tacotron.gta')
    with pytest.raises(SystemExit):
        G.main(['--gl-iters', '5'])
    assert G.gta_path('/x', '/d/wavs/LJ001-0001.wav')[:-len(G.SUFFIX)] + G.WAV_SUFFIX == os.path.join('/x', 'LJ001-0001.gta.wav')
