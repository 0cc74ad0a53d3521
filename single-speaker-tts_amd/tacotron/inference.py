"""Drop-in mirror of the reference's ``tacotron.inference`` (tacotron/inference.py).

``pad_sentence`` (:22-27), ``inference(model, sentences)`` (:30-105) and the body of
``__main__`` (:130-200) as :func:`synthesize_sentences`: ids -> padded batch -> network ->
de-normalise -> ``** magnitude_power`` -> Griffin-Lim -> ``{i+1}.wav``.

Where the reference fans Griffin-Lim out to 6 worker processes, one utterance each
(:185-188), the whole batch is reconstructed by one batched kernel sequence on the GPU.
"""
import json
import os

import numpy as np

from . import attention_check
from .._hip import (LOUDNESS_MAX_PEAK, loudness_setting, momentum_thousandths, phase_init_value, pitch_octaves_value, pitch_semitones_value,
                    silence_keep_frames, speaking_rate_value, stop_at_silence_setting)
from ..audio.conversion import ms_to_samples
from ..audio.io import save_wav
from .model import Mode, Tacotron
from .params import dataset_params, inference_params, model_params


def pad_sentence(_sentence, _max_len):
    """reference tacotron/inference.py:22-27."""
    pad_len = _max_len - len(_sentence)
    pad_token = dataset_params.vocabulary_dict['pad']
    return np.append(_sentence, [pad_token] * pad_len)


def inference(model, sentences, n_steps=None):
    """reference tacotron/inference.py:30-105.

    Arguments:
        model (Tacotron): model with restored weights.
        sentences: list/array of padded id sequences (B, T_sent).

    Returns:
        list of np.ndarray: per utterance the linear-scale magnitude spectrogram, shape
        (1025, T) float32 = decibel_to_magnitude(inv_normalize_decibel(spec.T, mel_ref_db,
        mel_max_db)) exactly as the reference (it uses the *mel* dB constants, :96-98).
    """
    sentences = np.asarray(sentences, dtype=np.int32)
    if inference_params.dump_alignments or inference_params.dump_linear_spectrogram:
        fetches = [model.summary(), model.output_linear_spec] \
            if os.path.isdir(inference_params.synthesis_dir) else [model.output_linear_spec]
    else:
        fetches = [model.output_linear_spec]
    out = model.predict_device(sentences, n_steps)
    if len(fetches) == 2:
        model._dump(out)
    loader = dataset_params.dataset_loader
    mag = model.engine.denorm_power(out['linear'], loader.mel_mag_ref_db, loader.mel_mag_max_db, 1.0).to_host()
    return [mag[b] for b in range(mag.shape[0])]


REPORT_FILE = 'alignment_report.json'   # what --check-alignment writes beside the wavs
SILENCE_KEEP_MS = 100.0   # audio kept behind the last frame above the threshold where a caller does not say


def stop_setting(hp, stop_at_silence_db, silence_keep_ms):
    """``stop_at_silence_db`` / ``silence_keep_ms`` of the helpers below as the engine's ``stop_at_silence``: None, or
    (threshold_db, keep_frames) with the milliseconds converted by ms_to_samples and the hop (rounded up to whole frames).
    The threshold is in de-normalised dB, the units ``audio.effects.silence_interval_from_spectrogram`` compares in."""
    if stop_at_silence_db is None:
        return None
    if not float(silence_keep_ms) >= 0.0:
        raise ValueError('silence_keep_ms must be >= 0, got {!r}'.format(silence_keep_ms))
    hp = getattr(hp, 'hparams', hp)   # (a model serves for its hyper-parameters: they are looked at only where stopping is asked for)
    hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    return stop_at_silence_setting((stop_at_silence_db, silence_keep_frames(ms_to_samples(float(silence_keep_ms), hp.sampling_rate), hop)))


def cut_waveforms(wavs, n_frames, hop):
    """Row b of a padded batch cut to its own hop (n_frames[b] - 1) samples: a list of arrays."""
    return [wavs[b][:hop * (int(n_frames[b]) - 1)] for b in range(len(n_frames))]


def pad_id():
    """the id the sentences are padded with (``pad_sentence``): what the attention diagnostics take the sentence lengths from"""
    return int(dataset_params.vocabulary_dict['pad'])


class SynthSettings(object):
    """The synthesis settings every helper of this layer takes, checked once -- ValueError before an engine is touched, in the
    order of ``_hip.SETTINGS`` -- and kept as the checked values ``momentum``, ``stop``, ``rate``, ``octaves``, ``phase_init``,
    ``loud`` and ``check_alignment``.  ``hp``: the hyper-parameters the stopping takes its hop from, or a model that has them.

    ``momentum``: fast Griffin-Lim (audio.synthesis), 0.0 = the reference's loop.
    ``stop_at_silence_db``: stop every utterance ``silence_keep_ms`` behind its last frame whose loudest bin is above that many
    dB (the reference's TODO at tacotron/inference.py:76-78); the waveforms of a batch are then a LIST of B arrays, each cut to its
    own length.
    ``speaking_rate``: 1.0 (None likewise), or a rate in [0.25, 4] -- the magnitudes are time-stretched ahead of Griffin-Lim (the
    reference's audio.effects.time_stretch, on the one reconstruction the call runs anyway): the waveforms are (B, hop*(T'-1))
    with T' = ceil(T / rate), ``init_phase`` is (B, F, T').
    ``pitch``: 0.0 (None likewise), or a shift in [-1, 1] octaves (the reference's audio.effects.pitch_shift on the same
    reconstruction: the magnitudes are stretched by rate * 2 ** -pitch and the resampler takes Griffin-Lim's samples back); the
    waveforms keep the shape they have without it, ``init_phase`` is (B, F, ceil(T / (rate * 2 ** -pitch))).
    ``pitch_semitones``: the same shift as the command line states it, in [-12, 12] semitones, in place of ``pitch``.
    ``phase_init``: 'random' (the reference's start, from ``seed``), 'estimate' (Griffin-Lim starts from phases estimated from
    the call's magnitudes, audio.synthesis; far fewer iterations are then needed) or None (the engine's ``gl_init`` option);
    an ``init_phase`` wins.
    ``loudness``: None (the engine's setting), a target in LUFS or ``(target_lufs, max_peak)`` -- every utterance is taken to that
    integrated loudness (ITU-R BS.1770-4, measured over the samples it holds) on the device instead of being peak-normalised.
    ``check_alignment``: the call also reduces its alignments to one record per utterance on the device
    (``Engine.alignment_stats``; the sentence lengths are taken from the ids' padding) and answers with the records and
    ``attention_check.verdict`` of every utterance, an empty tuple where the attention read the sentence cleanly."""

    def __init__(self, hp, momentum=0.0, stop_at_silence_db=None, silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0,
                 phase_init='random', loudness=None, check_alignment=False, pitch_semitones=None):
        momentum_thousandths(momentum)
        self.momentum = momentum
        self.stop = stop_setting(hp, stop_at_silence_db, silence_keep_ms)
        self.stop_at_silence_db, self.silence_keep_ms = stop_at_silence_db, silence_keep_ms
        self.rate = speaking_rate_value(1.0 if speaking_rate is None else speaking_rate)
        self.octaves = pitch_octaves_value(0.0 if pitch is None else pitch) if pitch_semitones is None else pitch_semitones_value(pitch_semitones)
        phase_init_value(phase_init)
        self.phase_init = phase_init
        self.loud = loudness_setting(loudness)
        self.check_alignment = check_alignment

    def engine_keywords(self):
        """the settings as ``Engine.synthesize`` / ``Engine.synthesize_host`` take them"""
        return dict(momentum=self.momentum, stop_at_silence=self.stop, speaking_rate=self.rate, pitch=self.octaves,
                    phase_init=self.phase_init, loudness=self.loud, alignment_stats=(True, pad_id()) if self.check_alignment else None)

    def keywords(self):
        """the settings as the helpers of this layer take them (``check_alignment`` apart, which not every one takes)"""
        return dict(momentum=self.momentum, stop_at_silence_db=self.stop_at_silence_db, silence_keep_ms=self.silence_keep_ms,
                    speaking_rate=self.rate, pitch=self.octaves, phase_init=self.phase_init, loudness=self.loud)


def synthesize_batch(model, sentences, n_steps=None, n_iter=None, init_phase=None, seed=0, peak_normalize=False,
                     momentum=0.0, stop_at_silence_db=None, silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0,
                     phase_init='random', loudness=None, check_alignment=False):
    """ids (B, T_sent) -> waveforms (B, hop*(T-1)) float32: inference() + the synthesize() closure
    of the reference (tacotron/inference.py:170-188) fused into one device call.  The settings from ``momentum`` on: as
    ``SynthSettings`` has them.  With ``stop_at_silence_db`` the result is a list of B waveforms, with ``check_alignment`` it is
    ``(waveforms, records, verdicts)``."""
    s = SynthSettings(model, momentum, stop_at_silence_db, silence_keep_ms, speaking_rate, pitch, phase_init, loudness, check_alignment)
    hp = model.hparams
    loader = dataset_params.dataset_loader
    win_len = ms_to_samples(hp.win_len, hp.sampling_rate)
    win_hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    S = n_steps or model.n_steps()
    out = model.engine.synthesize(np.ascontiguousarray(sentences, dtype=np.int32), S, loader.mel_mag_ref_db,
                                  loader.mel_mag_max_db, hp.magnitude_power,
                                  hp.reconstruction_iterations if n_iter is None else n_iter, win_len, win_hop,
                                  init_phase=init_phase, seed=seed, peak_normalize=peak_normalize, **s.engine_keywords())
    wavs = cut_waveforms(out['wav'].to_host(), out['n_frames'], win_hop) if s.stop is not None else out['wav'].to_host()
    if check_alignment:
        records = model.engine.synth_alignment_stats(len(sentences))
        return wavs, records, attention_check.verdict(records)
    return wavs


def synthesize_stream(model, batches, n_steps=None, n_iter=None, seed=0, peak_normalize=False, copy=False, want_linear=False,
                      want_alignments=False, momentum=0.0, stop_at_silence_db=None, silence_keep_ms=SILENCE_KEEP_MS,
                      speaking_rate=1.0, pitch=0.0, phase_init='random', loudness=None, check_alignment=False):
    """Generator over batches of padded id sequences (each (B, T_sent) int32, HOST arrays) -> per batch the waveforms
    (B, hop*(T-1)) float32 in host memory, with THREE batches in flight: batch k + 2 is uploaded and encoded, batch k + 1
    is in its decoder, batch k in its post-net / Griffin-Lim while batch k - 1 is being downloaded (the reference runs the
    batches one after the other, tacotron/inference.py:75-101,185-200).  The arrays yielded are views of the library's
    pinned buffers unless ``copy``: valid until two more batches have been requested.

    With ``want_linear`` / ``want_alignments`` every item is a tuple ``(wavs, linear, alignments)``: the normalised linear
    spectrograms (B, T, 1025) -- what ``model.output_linear_spec`` is, the thing the reference's ``inference()`` fetches
    (:75-92) -- and the alignments (n_steps, B, T_sent) of the same call, downloaded behind the waveforms (None where not
    asked for).  The settings from ``momentum`` on: as ``SynthSettings`` has them.  With ``stop_at_silence_db`` the waveforms
    of a batch are a list of B arrays (views of the pinned rows unless ``copy``), each cut to its own length.  With
    ``check_alignment`` every item additionally carries the batch's alignment records and verdicts, ``(wavs, records,
    verdicts)`` or ``(wavs, linear, alignments, records, verdicts)``; the 56 bytes per utterance come down with the waveforms."""
    # (a generator: a bad setting is refused at its first item, before the engine is touched)
    s = SynthSettings(model, momentum, stop_at_silence_db, silence_keep_ms, speaking_rate, pitch, phase_init, loudness, check_alignment)
    hp = model.hparams
    loader = dataset_params.dataset_loader
    win_len = ms_to_samples(hp.win_len, hp.sampling_rate)
    win_hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    S = n_steps or model.n_steps()
    it = hp.reconstruction_iterations if n_iter is None else n_iter
    eng = model.engine
    extra = want_linear or want_alignments

    def waveforms(ticket):
        if s.stop is None:
            return eng.wait_host(ticket, copy=copy)
        n_frames = eng.wait_host_frames(ticket)
        return cut_waveforms(eng.wait_host(ticket, copy=copy), n_frames, win_hop)

    def collect(ticket):
        checked = ()
        if check_alignment:
            records = eng.wait_host_alignment_stats(ticket)
            checked = (records, attention_check.verdict(records))
        if not extra:
            return ((waveforms(ticket),) + checked) if checked else waveforms(ticket)
        lin, ali = eng.wait_host_outputs(ticket, copy=copy)
        return (waveforms(ticket), lin, ali) + checked

    # three batches in flight (the library's three buffer sets): the encoder of batch k + 2 runs one inter-Griffin-Lim gap
    # ahead of its decoder, which follows the decoder of batch k + 1 without a pause, beside the Griffin-Lim of batch k
    pending = []
    for k, ids in enumerate(batches):
        pending.append(eng.synthesize_host(ids, S, loader.mel_mag_ref_db, loader.mel_mag_max_db, hp.magnitude_power, it, win_len,
                                           win_hop, seed=seed + k, peak_normalize=peak_normalize, want_linear=want_linear,
                                           want_alignments=want_alignments, **s.engine_keywords()))
        if len(pending) == 3:
            yield collect(pending.pop(0))
    while pending:
        yield collect(pending.pop(0))


def inference_stream(model, batches, n_steps=None, n_iter=None, seed=0, momentum=0.0, phase_init='random'):
    """``inference()`` over a stream of batches with three calls in flight: per batch ``(spectrograms, waveforms)`` where
    ``spectrograms`` is what the reference's ``inference()`` returns for that batch -- per utterance the (1025, T) linear
    magnitude spectrogram ``decibel_to_magnitude(inv_normalize_decibel(spec.T, mel_ref_db, mel_max_db))``
    (tacotron/inference.py:93-101; computed on the host from the downloaded network output with the conversions of
    ``audio.conversion``) -- and ``waveforms`` the Griffin-Lim reconstructions the reference's ``__main__`` makes of them
    (:170-188).  ``momentum`` and ``phase_init`` as in ``synthesize_stream``."""
    s = SynthSettings(None, momentum=momentum, phase_init=phase_init)
    loader = dataset_params.dataset_loader
    ref_db, max_db = np.float32(loader.mel_mag_ref_db), np.float32(loader.mel_mag_max_db)
    rng_db = np.float32(abs(float(ref_db)) + abs(float(max_db)))
    for wavs, lin, _ in synthesize_stream(model, batches, n_steps=n_steps, n_iter=n_iter, seed=seed, copy=True, want_linear=True,
                                          **s.keywords()):
        specs = []
        for b in range(lin.shape[0]):
            # inv_normalize_decibel, decibel_to_magnitude (reference audio/conversion.py:81-102, 32-53) in host arithmetic:
            # the device versions of audio.conversion would synchronise the stream that the next batch is running on
            db = (np.clip(lin[b].T, np.float32(0), np.float32(1)) - np.float32(1)) * rng_db + ref_db
            assert not (db < -100.0).any(), 'decibel_to_magnitude: values below -100 dB'
            specs.append(np.power(np.float32(10), db / np.float32(20)).astype(np.float32))
        yield specs, wavs


def synthesize_sentences(raw_sentences, weights, dataset=None, out_dir=None, device_id=0, seed=0, momentum=0.0,
                         stop_at_silence_db=None, silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0,
                         phase_init='random', loudness=None, check_alignment=False):
    """The reference's ``__main__`` (tacotron/inference.py:130-200) as a function.

    raw text lines -> process_sentences -> pad -> model -> wavs -> ``{i+1}.wav`` (peak-normalised
    float32 WAV, save_wav(norm=True)).  Returns the list of waveforms.  With ``stop_at_silence_db`` every file ends
    ``silence_keep_ms`` behind its utterance's last frame above that threshold instead of after max_iterations frames.
    The other settings from ``momentum`` on: as ``SynthSettings`` has them (a ``speaking_rate`` of 1.2: a fifth faster; a
    ``pitch`` of 4 / 12: four semitones up).  With a ``loudness`` the files hold the waveforms at that loudness, not
    peak-normalised.  With ``check_alignment`` the result is ``(waveforms, report)`` with ``report`` the list of ``{index,
    verdict, record}`` of ``attention_check.report``, also written to ``alignment_report.json`` beside the wavs."""
    # (ValueError before anything is loaded)
    s = SynthSettings(model_params, momentum, stop_at_silence_db, silence_keep_ms, speaking_rate, pitch, phase_init, loudness, check_alignment)
    from ..datasets.lj_speech import LJSpeechDatasetHelper
    out_dir = out_dir or inference_params.synthesis_dir
    if not os.path.isdir(out_dir):
        raise NotADirectoryError('The specified synthesis target folder does not exist.')
    dataset = dataset or LJSpeechDatasetHelper(dataset_folder=dataset_params.dataset_folder,
                                                char_dict=dataset_params.vocabulary_dict, fill_dict=False)
    id_sequences, sequence_lengths = dataset.process_sentences(raw_sentences)
    sentences = [np.frombuffer(s, dtype=np.int32) for s in id_sequences]
    max_length = max(sequence_lengths)
    sentences = np.array([pad_sentence(s, max_length) for s in sentences], dtype=np.int32)
    model = Tacotron(inputs=Tacotron.model_placeholders(), mode=Mode.PREDICT, weights=weights, device_id=device_id)
    wavs = synthesize_batch(model, sentences, seed=seed, peak_normalize=False, check_alignment=check_alignment, **s.keywords())
    report = None
    if check_alignment:
        wavs, records, _verdicts = wavs
        report = attention_check.report(records)
        with open(os.path.join(out_dir, REPORT_FILE), 'w') as f:
            json.dump(report, f, indent=1)
    for i, wav in enumerate(wavs):
        save_wav(os.path.join(out_dir, '{}.wav'.format(i + 1)), wav, model_params.sampling_rate, s.loud is None)
    return (list(wavs), report) if check_alignment else list(wavs)


def read_sentences(path):
    """reference tacotron/inference.py:139-143: one sentence per line, the newline removed (nothing else stripped)."""
    raw_sentences = []
    with open(path, 'r') as f_sent:
        for line in f_sent:
            raw_sentences.append(line.replace('\n', ''))
    return raw_sentences


def main(argv=None):
    """The reference's ``python tacotron/inference.py`` (tacotron/inference.py:130-200): read
    ``inference_params.synthesis_file``, restore the checkpoint named by ``inference_params`` (``checkpoint_file``, or the
    latest one of ``checkpoint_dir/checkpoint_load_run``: :44-55), synthesize, write ``{i+1}.wav`` into ``synthesis_dir``.

        python -m single-speaker-tts_amd.tacotron.inference [--synthesis-file F] [--synthesis-dir D]
                                                            [--weights CKPT | --synthetic-weights SEED]
                                                            [--momentum ALPHA]
                                                            [--stop-at-silence DB [--silence-keep-ms MS]]
                                                            [--rate R] [--pitch SEMITONES]
                                                            [--phase-init random|estimate]
                                                            [--loudness LUFS [--max-peak P]]
                                                            [--check-alignment]

    The options override the ``inference_params`` fields of the same name.  ``--weights`` takes what
    ``Tacotron.restore`` takes (a TensorFlow checkpoint prefix or run directory, or an ``.npz`` of the manifest's
    variables); ``--synthetic-weights`` a seed for the synthetic initialiser (no checkpoint ships with the reference).
    ``--stop-at-silence DB``: every wav ends ``--silence-keep-ms`` behind the last frame whose loudest bin is above DB
    (de-normalised dB, e.g. -40) instead of after the full max_iterations frames: files of different lengths.
    ``--rate R``: the speaking rate, 0.25 .. 4 (1.2: a fifth faster; default 1 = as the network speaks).
    ``--pitch SEMITONES``: the pitch, -12 .. 12 semitones (4: a major third up; default 0 = as the network speaks).
    ``--phase-init estimate``: Griffin-Lim starts from phases estimated from the magnitudes instead of random ones.
    ``--loudness LUFS``: every wav is taken to that integrated loudness (ITU-R BS.1770-4; -23: EBU R 128, -16: a common
    streaming level) with no sample beyond ``--max-peak`` (default 1), instead of being peak-normalised.
    ``--check-alignment``: the attention diagnostics (``tacotron.attention_check``) -- one JSON line per sentence (index,
    verdict, record) and ``alignment_report.json`` beside the wavs; the exit status stays 0 whatever the verdicts."""
    args = parse_args(argv)
    s = SynthSettings(model_params, args.momentum, args.stop_at_silence, args.silence_keep_ms, args.rate, pitch_semitones=args.pitch,
                      phase_init=args.phase_init, loudness=None if args.loudness is None else (args.loudness, args.max_peak),
                      check_alignment=args.check_alignment)
    out_dir = args.synthesis_dir or inference_params.synthesis_dir
    # Before we start doing anything we check if the required target folder actually exists (:131-133)
    if not os.path.isdir(out_dir):
        raise NotADirectoryError('The specified synthesis target folder does not exist.')
    raw_sentences = read_sentences(args.synthesis_file or inference_params.synthesis_file)
    print('{} sentences were loaded for inference.'.format(len(raw_sentences)))
    if args.synthetic_weights is not None:
        from .weights import synthetic_weights
        weights = synthetic_weights(args.synthetic_weights, model_params)
    elif args.weights is not None:
        weights = args.weights
    elif inference_params.checkpoint_file is not None:
        weights = inference_params.checkpoint_file
    else:
        weights = os.path.join(inference_params.checkpoint_dir, inference_params.checkpoint_load_run)
    wavs = synthesize_sentences(raw_sentences, weights, out_dir=out_dir, device_id=args.device, seed=args.seed,
                                check_alignment=args.check_alignment, **s.keywords())
    if args.check_alignment:
        wavs, report = wavs
        for row in report:
            print(json.dumps(row))
    for i in range(len(wavs)):
        print('Saved: "{}"'.format(os.path.join(out_dir, '{}.wav'.format(i + 1))))
    return 0


def parse_args(argv=None):
    """The command line of ``main``."""
    import argparse
    ap = argparse.ArgumentParser(prog='tacotron.inference')
    ap.add_argument('--synthesis-file', default=None)
    ap.add_argument('--synthesis-dir', default=None)
    ap.add_argument('--weights', default=None)
    ap.add_argument('--synthetic-weights', type=int, default=None)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--seed', type=int, default=0, help='seed of the Griffin-Lim start phases (the reference draws them unseeded)')
    ap.add_argument('--momentum', type=float, default=0.0,
                    help='fast Griffin-Lim momentum in [0, 1); 0 (default) is the reference\'s loop, librosa uses 0.99')
    ap.add_argument('--stop-at-silence', type=float, default=None, metavar='DB',
                    help='end every utterance behind its last frame above DB decibels (e.g. -40); default: all max_iterations frames')
    ap.add_argument('--silence-keep-ms', type=float, default=SILENCE_KEEP_MS, metavar='MS',
                    help='audio kept behind that frame (default {:g} ms)'.format(SILENCE_KEEP_MS))
    ap.add_argument('--rate', type=float, default=1.0, metavar='R',
                    help='speaking rate in [0.25, 4]: the magnitudes are time-stretched ahead of Griffin-Lim (1.2: a fifth faster; default 1)')
    ap.add_argument('--pitch', type=float, default=0.0, metavar='SEMITONES',
                    help='pitch shift in [-12, 12] semitones: the magnitudes are stretched and Griffin-Lim\'s samples resampled (default 0)')
    ap.add_argument('--phase-init', default='random', metavar='START',
                    help="Griffin-Lim's start phases: 'random' (default, the reference's) or 'estimate' (tracked from the magnitudes' peaks)")
    ap.add_argument('--loudness', type=float, default=None, metavar='LUFS',
                    help='integrated loudness (ITU-R BS.1770-4) every wav is taken to, e.g. -23; default: peak normalisation')
    ap.add_argument('--max-peak', type=float, default=LOUDNESS_MAX_PEAK, metavar='P',
                    help='with --loudness: the largest |sample| the gain may produce (default {:g})'.format(LOUDNESS_MAX_PEAK))
    ap.add_argument('--check-alignment', action='store_true',
                    help='attention diagnostics: one JSON line per sentence and {} beside the wavs'.format(REPORT_FILE))
    return ap.parse_args(argv)


if __name__ == '__main__':
    raise SystemExit(main())
