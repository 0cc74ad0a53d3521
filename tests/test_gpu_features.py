"""Dataset features on the GPU (csrc/features.hip) against the float64 restatement of the reference's load_audio
(datasets/lj_speech.py:106-156; tests/trim_oracle.py): trim bounds, feature parity, batch invariance, launch count, the
precalc entry point end to end, the effects, and the pass beside MFMA GEMM launches of another handle."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import feature_cases as FC
import trim_oracle as T
from conftest import ROOT, pkg
from feature_cases import speechlike
from neighbour_fixture import neighbour   # noqa: F401
from parity import assert_parity

pytestmark = pytest.mark.gpu
SR = 22050


def _batch(rng, B, lo=0.3, hi=3.0):
    wavs = []
    for b in range(B):
        n = int(rng.uniform(lo, hi) * SR)
        wavs.append(speechlike(rng, n, lead=int(rng.integers(0, 6000)), trail=int(rng.integers(0, 6000))))
    return wavs


@pytest.fixture(scope='module')
def eng():
    e = pkg().Engine()
    yield e
    e.close()


def _trim_cases(rng):
    cases = [
        speechlike(rng, 30001, lead=7000, trail=5003),          # both margins, lengths not multiples of the hop
        speechlike(rng, 20000, lead=9111),                       # leading silence only
        speechlike(rng, 17777, trail=8888),                      # trailing silence only
        speechlike(rng, 25013),                                  # no silence
        np.zeros(12345, np.float32),                             # all zeros: the whole recording
        speechlike(rng, 1030),                                   # n just above frame_length / 2
        speechlike(rng, 700, lead=400),                          # 1100 samples, a short burst
    ]
    return cases


@pytest.mark.parametrize('top_db', [40, 60])
def test_trim_bounds_equal_the_restatement(eng, top_db):
    wavs = _trim_cases(np.random.default_rng(top_db))
    for w in wavs:
        if np.any(w):
            assert T.threshold_margin(w, top_db) > 1e-3
    got = eng.trim_bounds(wavs, 2048, 512, top_db)
    ref = np.array([T.trim_bounds(w, top_db) for w in wavs])
    print('trim bounds', got.tolist())
    assert np.array_equal(got, ref)
    assert tuple(got[4]) == (0, 12345)


def test_trim_refuses_short_recordings(eng):
    with pytest.raises(pkg().TtsError, match='frame_length / 2'):
        eng.trim_bounds([np.ones(3000, np.float32), np.ones(1024, np.float32)])


def _check_features(got, w, label, **kw):
    mel_r, lin_r = T.features(w, **kw)
    mel_g, lin_g = got
    r = kw.get('r', 5)
    n_mels, F = mel_r.shape[1] // r, lin_r.shape[1] // r
    assert mel_g.shape == mel_r.shape and lin_g.shape == lin_r.shape, (mel_g.shape, mel_r.shape)
    for name, g, ref, C in (('mel', mel_g, mel_r, n_mels), ('lin', lin_g, lin_r, F)):
        g2, r2 = g.reshape(-1, C), ref.reshape(-1, C)
        assert_parity(g2, r2, {'frame': 0, 'channel': 1}, 1e-3, label + ' ' + name)
    # the reduction padding rows are exactly 0 (normalised or not)
    s, e = T.trim_bounds(w, kw.get('top_db', 60)) if kw.get('trim', True) else (0, len(w))
    hop = kw.get('hop', 275)
    Tf = 1 + (e - s) // hop
    assert not np.any(mel_g.reshape(-1, n_mels)[Tf:]) and not np.any(lin_g.reshape(-1, F)[Tf:])
    assert mel_g.reshape(-1, n_mels).shape[0] - Tf < r
    # every element inside the interval of feature_cases.py, with its exact checks (floor, padding rows)
    cfg = (kw.get('n_fft', 2048), kw.get('win', 1102), hop, kw.get('sr', SR), n_mels, kw.get('fmin', 0.0), kw.get('fmax', 8000.0))
    bad, _ = FC.check_rows(mel_g.reshape(-1, n_mels), lin_g.reshape(-1, F), FC.oracle(w, cfg, r, (s, e)), kw.get('normalize', True), label)
    assert not bad, bad


def test_feature_parity_model_configuration(eng):
    rng = np.random.default_rng(1)
    wavs = _batch(rng, 6, 0.5, 4.0)
    out = eng.extract_features(wavs)
    assert len(out) == 6
    for b, (w, got) in enumerate(zip(wavs, out)):
        assert got[0].shape[1] == 80 * 5 and got[1].shape[1] == 1025 * 5
        _check_features(got, w, 'model b%d' % b)


def test_feature_parity_statistics_configuration(eng):
    rng = np.random.default_rng(2)
    wavs = _batch(rng, 5, 0.3, 2.5)
    p = eng.feature_params(n_fft=1024, win_length=1024, hop_length=256, n_mels=80, fmin=0.0, fmax=float(SR // 2), normalize=0,
                           reduction=1, trim=0)
    out = eng.extract_features(wavs, p)
    for b, (w, got) in enumerate(zip(wavs, out)):
        _check_features(got, w, 'stats b%d' % b, n_fft=1024, win=1024, hop=256, fmax=float(SR // 2), normalize=False, r=1,
                        trim=False)


@pytest.mark.parametrize('n_fft,win,hop', [(512, 400, 100), (4096, 2400, 600), (2048, 1200, 300)])
def test_feature_parity_other_sizes(eng, n_fft, win, hop):
    rng = np.random.default_rng(n_fft + win)
    wavs = _batch(rng, 3, 0.5, 2.0)
    p = eng.feature_params(n_fft=n_fft, win_length=win, hop_length=hop)
    for b, (w, got) in enumerate(zip(wavs, eng.extract_features(wavs, p))):
        _check_features(got, w, '%d/%d/%d b%d' % (n_fft, win, hop, b), n_fft=n_fft, win=win, hop=hop)


def test_batch_invariance(eng):
    rng = np.random.default_rng(5)
    wavs = _batch(rng, 48, 0.3, 3.0)
    x = speechlike(rng, 40000, lead=3000, trail=2000)
    alone = eng.extract_features([x])[0]
    first = eng.extract_features([x] + wavs[1:])[0]
    last = eng.extract_features(wavs[:-1] + [x])[-1]
    for got in (first, last):
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1])


def test_launch_count_does_not_depend_on_the_batch(eng):
    rng = np.random.default_rng(6)
    wavs = _batch(rng, 48, 0.3, 3.0)
    eng.set_option('profile', 1)
    try:
        counts = []
        for batch in (wavs[:1], wavs):
            eng.profile_reset()
            eng.extract_features(batch)
            ms, n = eng.profile_get('features')
            print('features: B=%d %.3f ms, %d launches' % (len(batch), ms, n))
            counts.append(n)
    finally:
        eng.set_option('profile', 0)
    assert counts[0] == counts[1] == 3


def test_effects_agree_with_the_restatement(eng):
    E = pkg('audio.effects')
    audio = pkg('audio')
    previous = audio._default_engine          # (module-wide: later tests keep whatever engine they had)
    audio.set_default_engine(eng)
    try:
        rng = np.random.default_rng(8)
        w = speechlike(rng, 20000, lead=6000, trail=4000)
        s, e = T.trim_bounds(w, 40)
        assert T.threshold_margin(w, 40) > 1e-3
        y, idx = E.trim_silence(w)
        assert tuple(idx) == (s, e) and np.array_equal(y, w[s:e])
        y, n = E.crop_silence_left(w, SR, 100)
        assert n == min(int(0.1 * SR), s) and np.array_equal(y, w[n:])
        y, n = E.crop_silence_right(w, SR, 100)
        assert n == min(int(0.1 * SR), len(w) - e) and np.array_equal(y, w[:-n])
        y, n = E.crop_silence_left(w, SR, 100, safe_crop=False)
        assert n == int(0.1 * SR)
    finally:
        audio.set_default_engine(previous)


def _write_pcm16(path, x):
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(SR)
        f.writeframes(np.clip(np.round(x * 32767), -32768, 32767).astype('<i2').tobytes())


def test_precalc_entry_point_end_to_end(tmp_path):
    rng = np.random.default_rng(9)
    (tmp_path / 'wavs').mkdir()
    rows = []
    for i in range(5):
        _write_pcm16(tmp_path / 'wavs' / ('LJ%03d.wav' % i), speechlike(rng, int(rng.uniform(0.5, 2.5) * SR), 5000, 3000, -50.0, 1e-4))
        rows.append('LJ%03d|Text %d.|text number %d.' % (i, i, i))
    (tmp_path / 'metadata.csv').write_text('\n'.join(rows) + '\n')
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'single-speaker-tts_amd.tacotron.dataset_precalc_features', '--dataset-folder',
                        str(tmp_path), '--batch-size', '2'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    io = pkg('audio.io')
    DH = pkg('datasets.dataset_helper').DatasetHelper
    for i in range(5):
        wav_path = str(tmp_path / 'wavs' / ('LJ%03d.wav' % i))
        assert 'Writing: "{}"'.format(DH.feature_path(wav_path)) in r.stdout
        mel, lin = DH.load_features(wav_path)
        assert mel.dtype == np.float32 and lin.dtype == np.float32
        w, sr = io.load_wav(wav_path)
        assert sr == SR and T.threshold_margin(w) > 1e-3
        _check_features((mel, lin), w, 'npz %d' % i)


def test_features_beside_gemm_launches_of_another_handle(eng, neighbour):
    eng2, launch = neighbour
    wavs = _batch(np.random.default_rng(10), 16, 0.3, 2.0)
    configs = [None, eng.feature_params(n_fft=1024, win_length=1024, hop_length=256, normalize=0, reduction=1, trim=0)]
    for p in configs:
        quiet = eng.extract_features(wavs, p)
        bad = n = 0
        for _ in range(10):
            launch()
            outs = eng.extract_features(wavs, p)
            eng2.synchronize()
            for q, o in zip(quiet, outs):
                n += 1
                bad += not (np.array_equal(q[0], o[0]) and np.array_equal(q[1], o[1]))
        assert bad == 0, '%d of %d recordings differ from the quiet run' % (bad, n)


def test_decibel_statistics_match_the_restatement(eng, tmp_path):
    """datasets/statistics.py:11-98: per-file min / max of the raw dB spectrograms (n_fft 1024, hop 256, no trim), averaged."""
    S = pkg('datasets.statistics')
    rng = np.random.default_rng(12)
    paths, refs = [], []
    for i in range(3):
        p = tmp_path / ('s%d.wav' % i)
        _write_pcm16(p, speechlike(rng, int(rng.uniform(0.5, 2.0) * SR), 2000, 2000, -50.0, 1e-4))
        w, _ = pkg('audio.io').load_wav(str(p))
        mel, lin = T.features(w, n_fft=1024, win=1024, hop=256, fmax=float(SR // 2), normalize=False, r=1, trim=False)
        refs.append([lin.min(), lin.max(), mel.min(), mel.max()])
        paths.append(str(p))
    one = S.decibel_statistics(pkg('audio.io').load_wav(paths[0])[0], SR, engine=eng)
    assert np.allclose(one, refs[0], rtol=0, atol=2e-3), (one, refs[0])
    got = S.collect_decibel_statistics(paths, batch_size=2, engine=eng)
    print('decibel statistics', got.tolist())
    assert np.allclose(got, np.mean(refs, axis=0), rtol=0, atol=2e-3)
