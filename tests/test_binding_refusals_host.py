"""What the Python binding (_hip.py) refuses before it reaches the library, pinned: the exception type and the whole message of
every refusing call of the stages that take per-utterance lengths, strides or one-or-many waveforms, and of the shape refusals
of evaluate / teacher_forced.  The calls are made on an Engine that has no handle and no library.  The literals are the
binding's answers as they stood before its helpers were folded: a change of a helper that moves a message fails here.
The per-call synthesis settings go through every call that takes them; ``check_alignment`` has no refusal of its own (any true
value switches the diagnostics on): what it hands the engine is pinned in test_settings_host.py."""
import types

import numpy as np
import pytest

from conftest import pkg
from host_checks import no_device_engine

f32 = np.float32
WRAPPERS = ['eng.synthesize(IDS, *SYN, {0}=BAD)', 'eng.synthesize_host(IDS, *SYN, {0}=BAD)', 'I.synthesize_batch(None, IDS, {0}=BAD)',
            'next(I.synthesize_stream(None, [IDS], {0}=BAD))',
            "I.synthesize_sentences(['x'], '/nonexistent/weights', out_dir='/nonexistent', {0}=BAD)",
            "next(V.serve(iter([['x']]), '/nonexistent/weights', {0}=BAD))", 'V.post_process_spectrograms(LIN, None, {0}=BAD)']

# (the calls that take BAD, {the source of a bad value: the message every one of the calls answers it with})
GROUPS = [
    (['H.speaking_rate_value(BAD)', 'eng.stretch_magnitudes(MAG, BAD)', 'eng.stretch_rows(MAG, BAD)', 'eng.stretched_frames(4, BAD)',
      'eng.set_speaking_rate(BAD)', 'eng.time_stretch(np.zeros(4096, f32), BAD)'] + [w.format('speaking_rate') for w in WRAPPERS],
     dict({v: 'speaking_rate must be finite and lie in [0.25, 4], got ' + v for v in ('nan', '0', '0.2', '4.5', 'inf')},
          **{"'fast'": "speaking_rate must be a number in [0.25, 4], got 'fast'"})),
    (['H.stretch_frame_counts(BAD, 3, 12)', 'eng.stretch_magnitudes(MAG, 1.3, n_frames=BAD)', 'eng.stretch_rows(ROWS, 1.3, n_frames=BAD)'],
     {'[12, 7]': 'n_frames: shape (2,) for a batch of 3', '[[12, 7, 1]]': 'n_frames: shape (1, 3) for a batch of 3',
      '[12, 7, 1, 1]': 'n_frames: shape (4,) for a batch of 3', '12': 'n_frames: shape () for a batch of 3',
      '[12, 0, 1]': 'n_frames[1] = 0 is not in 1 .. T = 12', '[12, 13, 1]': 'n_frames[1] = 13 is not in 1 .. T = 12',
      '[12.0, 7.0, 1.0]': 'n_frames must be integers, got float64'}),
    (['H.resample_ratio_value(BAD)', 'H.resampled_length(10, BAD)', 'eng.resample(WAV, BAD)', 'eng.resampled_length(10, BAD)'],
     dict({v: 'the resampling ratio must be finite and lie in [0.25, 4], got ' + v for v in ('nan', 'inf', '0.0', '0.2', '4.5', '-1.0')},
          **{"'fast'": "the resampling ratio must be a number in [0.25, 4], got 'fast'"})),
    (['H.pitch_octaves_value(BAD)', 'eng.set_pitch(BAD)', 'eng.pitch_shift(np.zeros(4096, f32), 22050, BAD)'] + [w.format('pitch') for w in WRAPPERS],
     dict({v: 'pitch must be finite and lie in [-1, 1] octaves, got ' + v for v in ('nan', 'inf', '1.5', '-1.01')},
          **{"'high'": "pitch must be a number of octaves in [-1, 1], got 'high'"})),
    (['eng.resample(WAV, 2.0, n_samples=BAD)'],
     {'[20, 7]': 'n_samples: 3 integers are needed, got shape (2,) of int64', '[[20, 7, 1]]': 'n_samples: 3 integers are needed, got shape (1, 3) of int64',
      '20': 'n_samples: 3 integers are needed, got shape () of int64', '[20, 0, 1]': 'n_samples[1] = 0 is not in 1 .. n = 20',
      '[20, 21, 1]': 'n_samples[1] = 21 is not in 1 .. n = 20', '[20.0, 7.0, 1.0]': 'n_samples: 3 integers are needed, got shape (3,) of float64'}),
    (['H.phase_init_value(BAD)', 'eng.griffin_lim(GMAG, 2, 1102, 275, 2048, phase_init=BAD)',
      'Y.griffin_lim_v2(GMAG[0], 1102, 275, 2048, 2, engine=eng, phase_init=BAD)',
      'Y.spectrogram_to_wav(GMAG[0], 1102, 275, 2048, 2, engine=eng, phase_init=BAD)',
      'next(I.inference_stream(None, [IDS], phase_init=BAD))'] + [w.format('phase_init') for w in WRAPPERS],
     {v: "phase_init must be None, 'random' or 'estimate', got " + v for v in ("'Estimate'", "'spsi'", "''", '1', '0', 'True', '1.0', "b'estimate'")}),
    (['eng.phase_estimate(PMAG, *BAD)'],
     dict({'({}, 64)'.format(v): 'phase_estimate: n_fft must be a power of two between 256 and 4096, got ' + v for v in ('250', '128', '8192', '256.5')},
          **{'(256, 0)': 'phase_estimate: need 1 <= hop_length <= n_fft, got 0', '(256, 257)': 'phase_estimate: need 1 <= hop_length <= n_fft, got 257',
             '(256, 1.5)': 'phase_estimate: need 1 <= hop_length <= n_fft, got 1.5', '(512, 64)': 'phase_estimate: 129 bins given, n_fft = 512 has 257'})),
    (['eng.phase_estimate(PMAG, 256, 64, n_frames=BAD)'],
     {'[10, 7]': 'n_frames: shape (2,) for a batch of 3', '[[10, 7, 1]]': 'n_frames: shape (1, 3) for a batch of 3', '10': 'n_frames: shape () for a batch of 3',
      '[10, 0, 1]': 'n_frames[1] = 0 is not in 1 .. T = 10', '[10, 11, 1]': 'n_frames[1] = 11 is not in 1 .. T = 10',
      '[10.0, 7.0, 1.0]': 'n_frames must be integers, got float64'}),
    # the per-call synthesis settings: every keyword through every call that takes it
    (['H.momentum_thousandths(BAD)', 'eng.griffin_lim(GMAG, 2, 1102, 275, 2048, momentum=BAD)',
      'Y.griffin_lim_v2(GMAG[0], 1102, 275, 2048, 2, engine=eng, momentum=BAD)',
      'next(I.inference_stream(None, [IDS], momentum=BAD))'] + [w.format('momentum') for w in WRAPPERS],
     dict({v: 'momentum must be in [0, 1), got ' + v for v in ('nan', '1.0', '-0.1', '1.5', 'inf')},
          **{"'fast'": "could not convert string to float: 'fast'"})),
    (['H.stop_at_silence_setting(BAD)'] + [w.format('stop_at_silence') for w in WRAPPERS[:2]],
     dict({v: 'stop_at_silence must be None or (threshold_db, keep_frames), got ' + v for v in ('5', "'quiet'", '(-30.0, 2, 1)', '(-30.0,)')},
          **{'(nan, 2)': 'stop_at_silence: threshold_db is NaN', '(-30.0, -1)': 'stop_at_silence: keep_frames must be an integer >= 0, got -1',
             '(-30.0, 1.5)': 'stop_at_silence: keep_frames must be an integer >= 0, got 1.5'})),
    (['H.loudness_setting(BAD)', 'eng.set_loudness(BAD)'] + [w.format('loudness') for w in WRAPPERS],
     dict({v: 'loudness must be None, a target in LUFS or (target_lufs, max_peak), got ' + v for v in ('(-23.0,)', '(-23.0, 1.0, 2.0)')},
          **{"'loud'": "loudness: target_lufs and max_peak must be numbers, got 'loud', 1.0",
             "(-23.0, 'x')": "loudness: target_lufs and max_peak must be numbers, got -23.0, 'x'",
             'nan': 'loudness: the target must be a finite number of LUFS, got nan', 'inf': 'loudness: the target must be a finite number of LUFS, got inf',
             '(-23.0, 0.0)': 'loudness: max_peak must be finite and positive, got 0.0', '(-23.0, nan)': 'loudness: max_peak must be finite and positive, got nan'})),
    (['H.alignment_stats_setting(BAD)'] + [w.format('alignment_stats') for w in WRAPPERS[:2]],
     dict({v: 'alignment_stats must be None, a bool or (enabled, pad_id), got ' + v for v in ('3', "'on'", '(True,)', '(True, 1.5)', '(1, 0)', '(True, 0, 0)', '1.0')},
          **{'(True, 2 ** 31)': 'alignment_stats must be None, a bool or (enabled, pad_id), got (True, 2147483648)'})),
    # ... and this layer's own two, through the five calls above the engine (a model that has hyper-parameters and nothing else)
    ([w.replace('(None, ', '(M, ').format('stop_at_silence_db') for w in WRAPPERS[2:]],
     {'nan': 'stop_at_silence: threshold_db is NaN', "'quiet'": "could not convert string to float: 'quiet'", "''": "could not convert string to float: ''"}),
    ([w.replace('(None, ', '(M, ').format('stop_at_silence_db=-40.0, silence_keep_ms') for w in WRAPPERS[2:]],
     dict({v: 'silence_keep_ms must be >= 0, got ' + v for v in ('-1.0', 'nan', '-inf')}, **{"'long'": "could not convert string to float: 'long'"})),
]

F0_LAGS = ' are not 2 <= tau_min <= tau_max <= 1024 (tts_f0_max_lag): fmin is at least sampling_rate / 1024'
F0_INTS = 'f0: hop_length >= 1, window and the lags must be integers, got '
F0_RATES = 'f0: need a positive finite sampling rate and 0 < fmin <= fmax, got '
F0C_SHAPES = 'f0_compare: (B, Ta) and (B, Tb) tracks and a (B, rows, 2) path are needed, got shapes '
MFCC_N = 'mfcc: need 1 <= n_mfcc <= n_mels <= 1024, got n_mfcc = '
DTW_D = 'dtw: need 1 <= D and skip + D <= the row length, got D = '
SINGLE = [
    # speaking rate
    ('eng.stretch_magnitudes(MAG, 1.3, n_frames=[12, 7, 1], T_out=9)', 'stretch_magnitudes: T_out = 9 is smaller than the longest stretched utterance, 10 frames'),
    ('eng.stretch_magnitudes(np.ones((5, 12), f32), 1.3)', 'stretch_magnitudes: a non-empty 3-D array is needed, got shape (5, 12)'),
    ('eng.stretch_rows(ROWS, 1.3, row_stride=4)', 'stretch_rows: row_stride 4 < F = 5'),
    ('eng.stretch_rows(ROWS[0], 1.3)', 'stretch_rows: a non-empty 3-D array is needed, got shape (12, 5)'),
    ('eng.stretch_rows(ROWS, 1.3, T_out=3)', 'stretch_rows: T_out = 3 is smaller than the longest stretched utterance, 10 frames'),
    ('eng.time_stretch(np.zeros((2, 3, 4), f32), 1.2)', 'time_stretch: one waveform (n,) or a uniform batch (B, n) is needed, got shape (2, 3, 4)'),
    ('eng.time_stretch(np.zeros(600, f32), 2.0)', 'time_stretch: 600 samples at rate 2.0 leave a signal shorter than n_fft / 2'),
    # resampling and pitch
    ('eng.resample(np.zeros((2, 3, 4), f32), 2.0)', 'resample: one waveform (n,) or a batch (B, n) is needed, got shape (2, 3, 4)'),
    ('eng.resample(WAV, 2.0, N_out=0)', 'resample: N_out = 0 < 1'),
    ('eng.resample(WAV[0], 2.0, n_samples=[20, 7])', 'n_samples: 1 integers are needed, got shape (2,) of int64'),
    ('H.pitch_frames(40, 2.5, -1.0)', 'speaking rate 2.5 times 2 ** --1.0 octaves = 5.0 is outside [0.25, 4]'),
    ('H.pitch_frames(40, 0.4, 1.0)', 'speaking rate 0.4 times 2 ** -1.0 octaves = 0.2 is outside [0.25, 4]'),
    ('V.post_process_spectrograms(LIN, None, speaking_rate=2.5, pitch=-1.0)', 'speaking rate 2.5 times 2 ** --1.0 octaves = 5.0 is outside [0.25, 4]'),
    ('V.post_process_spectrograms(LIN, None, speaking_rate=0.4, pitch=1.0)', 'speaking rate 0.4 times 2 ** -1.0 octaves = 0.2 is outside [0.25, 4]'),
    # estimated phases and the end of speech
    ('eng.phase_estimate(np.ones((129, 10), f32), 256, 64)', 'phase_estimate: a non-empty 3-D array is needed, got shape (129, 10)'),
    ('eng.phase_estimate_rows(PROWS, 256, 64, row_stride=128)', 'phase_estimate_rows: row_stride 128 < F = 129'),
    ('eng.phase_estimate_rows(PMAG, 256, 64)', 'phase_estimate: 10 bins given, n_fft = 256 has 129'),
    ('eng.phase_estimate_rows(PROWS, 256, 64, n_frames=[10, 11, 1])', 'n_frames[1] = 11 is not in 1 .. T = 10'),
    ('eng.speech_frames(PROWS[0], 0.5)', 'speech_frames: spec must be (B, T, F), got shape (10, 129)'),
    # F0 (its n_samples borrow the n_frames wording)
    ('eng.f0(X, 22050, 275, window=2049)', 'f0: window = 2049 is not in 1 .. 2048 (tts_f0_max_window)'),
    ('eng.f0(X, 22050, 275, fmin=20.0)', 'f0: the lags 44 .. 1103' + F0_LAGS),
    ('eng.f0(X, 22050, 275, tau_min=80, tau_max=70)', 'f0: the lags 80 .. 70' + F0_LAGS),
    ('eng.f0(X, 22050, hop_length=0)', F0_INTS + '0, 1024, 44, 368'),
    ('eng.f0(X, 22050, hop_length=2.5)', F0_INTS + '2.5, 1024, 44, 368'),
    ('eng.f0(X, 22050, 275, window=0)', 'f0: window = 0 is not in 1 .. 2048 (tts_f0_max_window)'),
    ('eng.f0(X, 22050, 275, threshold=nan)', 'f0: the threshold is NaN'),
    ('eng.f0(X, 22050, 275, fmin=0.0)', F0_RATES + '22050, 0.0, 500.0'),
    ('eng.f0(X, 22050, 275, fmax=50.0)', F0_RATES + '22050, 60.0, 50.0'),
    ('eng.f0(X, nan, 275)', F0_RATES + 'nan, 60.0, 500.0'),
    ('eng.f0(X, 22050, 275, n_samples=[5000, 0])', 'n_frames[1] = 0 is not in 1 .. T = 5000'),
    ('eng.f0(X, 22050, 275, n_samples=[5000, 5001])', 'n_frames[1] = 5001 is not in 1 .. T = 5000'),
    ('eng.f0(X, 22050, 275, n_samples=[5000])', 'n_frames: shape (1,) for a batch of 2'),
    ('eng.f0(np.zeros((1, 2, 3), f32), 22050, 275)', 'f0: one waveform (n,) or a batch (B, n) is needed, got shape (1, 2, 3)'),
    ('eng.f0_compare(FA[0], FB, PATH)', F0C_SHAPES + '(40,), (2, 55) and (2, 94, 2)'),
    ('eng.f0_compare(FA, FB[:1], PATH)', 'f0_compare: 2 tracks in f0_a, 1 in f0_b and 2 paths'),
    ('eng.f0_compare(FA, FB, PATH[:, :, :1])', F0C_SHAPES + '(2, 40), (2, 55) and (2, 94, 1)'),
    ('eng.f0_compare(FA, FB, PATH[:1])', 'f0_compare: 2 tracks in f0_a, 2 in f0_b and 1 paths'),
    ('eng.f0_compare(FA, FB, PATH[0])', F0C_SHAPES + '(2, 40), (2, 55) and (94, 2)'),
    # cepstra and alignment
    ('eng.mfcc(MEL, 0)', MFCC_N + '0, n_mels = 80'),
    ('eng.mfcc(MEL, 81)', MFCC_N + '81, n_mels = 80'),
    ('eng.mfcc(MEL, 2.5)', MFCC_N + '2.5, n_mels = 80'),
    ('eng.mfcc(MEL[0], 13)', 'mfcc: rows must be a non-empty (B, T, n_mels) array, got shape (12, 80)'),
    ('eng.mfcc(MEL, 13, row_stride=79)', 'mfcc: row_stride 79 < n_mels = 80'),
    ('eng.mfcc(MEL, 13, n_frames=[12, 0, 1])', 'n_frames[1] = 0 is not in 1 .. T = 12'),
    ('eng.mfcc(MEL, 13, n_frames=[12, 13, 1])', 'n_frames[1] = 13 is not in 1 .. T = 12'),
    ('eng.mfcc(MEL, 13, n_frames=[12, 1])', 'n_frames: shape (2,) for a batch of 3'),
    ('eng.mfcc(MEL, 13, n_frames=[1.0, 2.0, 3.0])', 'n_frames must be integers, got float64'),
    ('eng.dtw(A, B[:2])', 'dtw: 3 sequences in a and 2 in b'),
    ('eng.dtw(A[0], B[0])', 'dtw: a and b must be non-empty (B, T, K) arrays, got shapes (12, 14) and (20, 14)'),
    ('eng.dtw(A, B, D=0, skip=0)', DTW_D + '0, skip = 0, rows of 14 and 14'),
    ('eng.dtw(A, B, D=15, skip=0)', DTW_D + '15, skip = 0, rows of 14 and 14'),
    ('eng.dtw(A, B, D=14, skip=1)', DTW_D + '14, skip = 1, rows of 14 and 14'),
    ('eng.dtw(A, B, D=1.5, skip=0)', DTW_D + '1.5, skip = 0, rows of 14 and 14'),
    ('eng.dtw(A, B, D=1, skip=-1)', 'dtw: skip must be >= 0'),
    ('eng.dtw(A, B, n_a=[12, 13, 1])', 'n_frames[1] = 13 is not in 1 .. T = 12'),
    ('eng.dtw(A, B, n_b=[20, 0, 1])', 'n_frames[1] = 0 is not in 1 .. T = 20'),
    # evaluation and teacher forcing: reduction 5, 80 mels, n_fft 2048
    ('eng.evaluate(IDS, TMEL[:1], TLIN)', 'evaluate: mel target of shape (1, 3, 400) for B = 2, r * n_mels = 400'),
    ('eng.evaluate(IDS, TMEL[:, :, :399], TLIN)', 'evaluate: mel target of shape (2, 3, 399) for B = 2, r * n_mels = 400'),
    ('eng.evaluate(IDS, TMEL, TLIN[:1])', 'evaluate: linear target of shape (1, 15, 1025), (2, 15, 1025) floats needed'),
    ('eng.evaluate(IDS, TMEL, TLIN[:, :14])', 'evaluate: linear target of shape (2, 14, 1025), (2, 15, 1025) floats needed'),
    ('eng.teacher_forced(IDS, TMEL[:1], TLIN)', 'teacher_forced: mel target of shape (1, 3, 400) for B = 2, r * n_mels = 400'),
    ('eng.teacher_forced(IDS, TMEL[:, :, :399])', 'teacher_forced: mel target of shape (2, 3, 399) for B = 2, r * n_mels = 400'),
    ('eng.teacher_forced(IDS, TMEL[:, :0])', 'teacher_forced: mel target of shape (2, 0, 400) for B = 2, r * n_mels = 400'),
    ('eng.teacher_forced(IDS, TMEL, TLIN[:1])', 'teacher_forced: linear target of shape (1, 15, 1025), (2, 15, 1025) floats needed'),
    ('eng.teacher_forced(IDS, TMEL, TLIN[:, :14])', 'teacher_forced: linear target of shape (2, 14, 1025), (2, 15, 1025) floats needed'),
    ('eng.decoder_forward_teacher(np.zeros((2, 5, 256), f32), TMEL[:1])', 'decoder_forward_teacher: mel target of shape (1, 3, 400) for B = 2, r * n_mels = 400'),
]


@pytest.fixture(scope='module')
def names():
    H = pkg('_hip')
    eng = no_device_engine()
    eng.cfg = H.TtsConfig(reduction=5, n_mels=80, n_fft=2048, vocabulary_size=40)
    return dict(H=H, eng=eng, np=np, f32=f32, I=pkg('tacotron.inference'), V=pkg('tacotron.serve'), Y=pkg('audio.synthesis'),
                nan=float('nan'), inf=float('inf'), IDS=np.ones((2, 5), np.int32), SYN=(2, 6.02, 99.89, 1.3, 2, 1102, 275),
                MAG=np.ones((3, 5, 12), f32), ROWS=np.ones((3, 12, 5), f32), LIN=np.zeros((1, 40, 1025), f32), WAV=np.zeros((3, 20), f32),
                PMAG=np.ones((3, 129, 10), f32), PROWS=np.ones((3, 10, 129), f32), MEL=np.ones((3, 12, 80), f32),
                A=np.ones((3, 12, 14), f32), B=np.ones((3, 20, 14), f32), X=np.zeros((2, 5000), f32), FA=np.zeros((2, 40), f32),
                FB=np.zeros((2, 55), f32), PATH=np.zeros((2, 94, 2), np.int32), GMAG=np.ones((1, 1025, 12), f32),
                TMEL=np.zeros((2, 3, 400), f32), TLIN=np.zeros((2, 15, 1025), f32), M=types.SimpleNamespace(hparams=pkg('tacotron.params').model_params))


def _refusal(call, names):
    with pytest.raises(Exception) as caught:
        eval(call, names)
    return type(caught.value), str(caught.value)


def test_every_refusal_keeps_its_type_and_text(names):
    n = 0
    for call, message in SINGLE:
        assert _refusal(call, names) == (ValueError, message), call
        n += 1
    for calls, answers in GROUPS:
        for bad, message in answers.items():
            for call in calls:
                assert _refusal(call, dict(names, BAD=eval(bad, names))) == (ValueError, message), (call, bad)
                n += 1
    assert n == len(SINGLE) + 6 * 13 + 7 * 3 + 7 * 4 + 5 * 10 + 6 + 8 * 12 + 8 + 6 + 6 * 11 + 7 * 3 + 8 * 9 + 8 * 3 + 3 * 5 + 4 * 5
