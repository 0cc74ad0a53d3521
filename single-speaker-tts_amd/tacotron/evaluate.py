"""Drop-in mirror of the reference's ``tacotron.evaluate`` (tacotron/evaluate.py): the eval loss of a checkpoint.

``batched_placeholders`` (:18-151) buckets the evaluation set by sentence length and pads every batch,
``evaluate`` (:153-257) runs ``Tacotron(..., Mode.EVAL)`` over one epoch and averages the three losses
unweighted over the batches, ``collect_checkpoint_paths`` (:284-326) lists a run's checkpoints and
:func:`main` is the reference's ``__main__`` (:329-364): the latest checkpoint, or with ``--all`` every one.

Batch order.  The reference fills its buckets from TensorFlow input queues, whose order is not reproducible.
Here the order is fixed: the buckets in ascending order of length, within a bucket the utterances in dataset
order, a batch whenever a bucket holds ``batch_size`` utterances; with ``allow_smaller_batches`` the leftovers of
the buckets then follow, in ascending bucket order, as smaller batches (without it they are dropped, as
TensorFlow drops them).  Because the losses are averaged per batch, the batch composition -- not the order --
decides the result.

Mel-cepstral distortion.  With ``mcd`` (``--mcd``) every utterance's free-running mel prediction is also compared with its
target along a dynamic-time-warping path (``audio.metrics.mel_cepstral_distortion``): a measure of the spectra that does not
count a prediction that speaks a little faster or slower than the recording as wrong at every frame.  The target side is the
utterance's unpadded ``ph_time_frames * r`` frames; the prediction side the same count, or with ``mcd_stop_at_silence``
(``--mcd-stop-at-silence DB``) the frames up to the last one of the predicted linear spectrogram that rises above that level.

F0 errors.  With ``f0`` (``--f0``) the prosody is measured along the same path: the predicted and the target linear spectrograms of
a batch both go through the same vocoder -- the de-normalisation, ``** magnitude_power`` and the ragged Griffin-Lim at the
lengths the distortion uses -- so that its colouring cancels, tts_f0 tracks both waveforms, and ``audio.metrics.f0_errors`` gives
every utterance its F0 RMSE in cents and Hz, its voicing error and its gross pitch error.  The path is computed whether or not
``mcd`` reports its figure.

Intelligibility.  With ``stoi`` (``--stoi``, ``--estoi`` for the extended form) every batch is also run teacher-forced
(``Tacotron.teacher_forced_device``), so that prediction and target are aligned frame by frame; the predicted and the target linear
spectrograms go through the same ragged Griffin-Lim -- one seed, one set of frame counts, as ``batch_f0`` does -- and
``audio.metrics.stoi`` compares the two waveforms (tts_stoi behind the resampler): ``metric/stoi`` or ``metric/estoi``, the mean
over the utterances with a finite figure, and ``stoi_utterances``, their count.

TensorBoard events are not written: every evaluated checkpoint appends one JSON line with the reference's
summary tags (``loss/loss``, ``loss/loss_decoder``, ``loss/loss_post_processing``) and its global step to
``<checkpoint_dir>/<checkpoint_save_run>/eval_summaries.jsonl``.
"""
import bisect
import json
import os

import numpy as np

from .model import Mode, Tacotron
from .params import LJSpeechConstants, dataset_params, evaluation_params, model_params

SUMMARY_FILE = 'eval_summaries.jsonl'


def bucket_boundaries(sentence_lengths, n_buckets):
    """reference :80-99: the first length of every ``n // n_buckets``-th slice of the sorted lengths, without the
    first and last one, de-duplicated.  AssertionError when fewer than ``n_buckets`` entries were loaded."""
    n_samples = len(sentence_lengths)
    if n_samples < n_buckets:
        raise AssertionError('The number of entries loaded is smaller than the number of '
                             'buckets to be created. Automatic calculation of the bucket '
                             'boundaries is not possible.')
    bucket_step = n_samples // n_buckets
    boundaries = np.sort(np.asarray(sentence_lengths))[::bucket_step][1:-1].tolist()
    return sorted(set(boundaries))


def bucket_batches(sentence_lengths, boundaries, batch_size, allow_smaller_batches=True):
    """Index lists of the batches in the documented order (module docstring).  An utterance of length L goes to bucket
    ``bisect_right(boundaries, L)``: buckets [-inf, b0), [b0, b1), ..., [b_last, inf) as in TensorFlow's
    bucket_by_sequence_length."""
    buckets = [[] for _ in range(len(boundaries) + 1)]
    for i, length in enumerate(sentence_lengths):
        buckets[bisect.bisect_right(boundaries, int(length))].append(i)
    full, rest = [], []
    for b in buckets:
        n_full = len(b) // batch_size
        full += [b[k * batch_size:(k + 1) * batch_size] for k in range(n_full)]
        if len(b) % batch_size:
            rest.append(b[n_full * batch_size:])
    return full + (rest if allow_smaller_batches else [])


def pad_batch(sentences, sentence_lengths, features):
    """dynamic_pad: ids padded with the <PAD> id 0, spectrograms with zero frames to the batch maximum.
    sentences: list of int32 arrays; features: list of (mel (T_red, n_mels*r), linear (T_red, F*r))."""
    B = len(sentences)
    Ts = max(len(s) for s in sentences)
    T_red = max(m.shape[0] for m, _ in features)
    ids = np.zeros((B, Ts), np.int32)
    mel = np.zeros((B, T_red, features[0][0].shape[1]), np.float32)
    lin = np.zeros((B, T_red, features[0][1].shape[1]), np.float32)
    frames = np.zeros(B, np.int32)
    for b, (s, (m, l)) in enumerate(zip(sentences, features)):
        ids[b, :len(s)] = s
        mel[b, :m.shape[0]] = m
        lin[b, :l.shape[0]] = l
        frames[b] = m.shape[0]
    return {
        'ph_sentences': ids,
        'ph_sentence_length': np.asarray(sentence_lengths, np.int32),
        'ph_mel_specs': mel,
        'ph_lin_specs': lin,
        'ph_time_frames': frames,
    }


def batched_placeholders(dataset, max_samples, batch_size, n_buckets=None, allow_smaller_batches=None, verbose=True):
    """reference :18-151: yields one padded feed dict per batch (keys ``ph_sentences`` (B, T_sent) int32,
    ``ph_sentence_length`` (B,), ``ph_mel_specs`` (B, T_red, n_mels*r), ``ph_lin_specs`` (B, T_red, F*r),
    ``ph_time_frames`` (B,) = unpadded T_red), in the order of the module docstring.  The features of a batch are
    read from the pre-computed ``.npz`` files when the batch is formed."""
    n_buckets = evaluation_params.n_buckets if n_buckets is None else n_buckets
    allow = evaluation_params.allow_smaller_batches if allow_smaller_batches is None else allow_smaller_batches
    sentences, sentence_lengths, wav_paths = dataset.load(max_samples=max_samples)
    if verbose:
        print('Loaded {} dataset entries.'.format(len(sentence_lengths)))
    boundaries = bucket_boundaries(sentence_lengths, n_buckets)
    if verbose:
        print('bucket_boundaries', boundaries)
        print('n_buckets: {} + 2'.format(len(boundaries)))
    for idx in bucket_batches(sentence_lengths, boundaries, batch_size, allow):
        yield pad_batch([np.frombuffer(sentences[i], dtype=np.int32) for i in idx],
                        [sentence_lengths[i] for i in idx],
                        [dataset.load_audio(wav_paths[i]) for i in idx])


def global_step_of(checkpoint_file):
    """reference :180: the global step is the part of the file name after the last '-'."""
    return int(checkpoint_file.split('-')[-1])


def batch_mcd(model, feed, out, mcd_coeffs=13, mcd_stop_at_silence=None):
    """The mel-cepstral distortion of every utterance of one evaluated batch: ``out`` is what ``evaluate_device`` returned for
    ``feed`` (its ``mel``, and with ``mcd_stop_at_silence`` its ``linear``).  -> (B,) float64"""
    return batch_alignment(model, feed, out, mcd_coeffs, mcd_stop_at_silence)[0]['mcd']


def batch_alignment(model, feed, out, mcd_coeffs=13, mcd_stop_at_silence=None, want_path=False):
    """The distortion of :func:`batch_mcd` with what it was measured on: (the dict of ``mel_cepstral_distortion`` -- with
    ``want_path`` its ``path`` --, the prediction's frame counts, the target's frame counts)."""
    from ..audio.metrics import mel_cepstral_distortion
    eng = model.engine
    r, nm = eng.cfg.reduction, eng.cfg.n_mels
    B = feed['ph_sentences'].shape[0]
    target = np.ascontiguousarray(feed['ph_mel_specs'], dtype=np.float32).reshape(B, -1, nm)
    n_target = np.asarray(feed['ph_time_frames'], np.int32) * r
    n_pred = n_target
    if mcd_stop_at_silence is not None:
        thr = eng.speech_threshold(mcd_stop_at_silence, LJSpeechConstants.linear_ref_db, LJSpeechConstants.linear_mag_max_db)
        n_frames, last = eng.speech_frames(out['linear'], thr, keep_frames=0, min_frames=1)
        n_pred = n_frames.to_host()
        n_frames.free()
        last.free()
    res = mel_cepstral_distortion(out['mel'], target, n_a=n_pred, n_b=n_target, n_coeffs=mcd_coeffs,
                                  ref_db=LJSpeechConstants.mel_mag_ref_db, max_db=LJSpeechConstants.mel_mag_max_db, engine=eng,
                                  want_path=want_path)
    return res, np.asarray(n_pred, np.int32), np.asarray(n_target, np.int32)


F0_KEYS = ('f0_rmse_cents', 'f0_rmse_hz', 'vuv_error', 'gross_pitch_error')


def batch_f0(model, feed, out, path, n_pred, n_target, f0_iters=None, f0_min=60.0, f0_max=500.0, seed=0):
    """The F0 errors of every utterance of one evaluated batch along ``path`` (B, 2 T - 1, 2), the alignment of
    :func:`batch_alignment` at the frame counts ``n_pred`` / ``n_target``: the predicted linear spectrogram ``out['linear']`` and
    the target's both become waveforms through the same vocoder and tracks through tts_f0.  -> the dict of
    ``audio.metrics.f0_errors``, or None where the batch is shorter than the vocoder's shortest signal."""
    from ..audio.metrics import f0_errors
    from ..audio.conversion import ms_to_samples
    eng, hp = model.engine, model.hparams
    loader = dataset_params.dataset_loader
    win_len, hop = ms_to_samples(hp.win_len, hp.sampling_rate), ms_to_samples(hp.win_hop, hp.sampling_rate)
    B = feed['ph_sentences'].shape[0]
    F = 1 + hp.n_fft // 2
    target = np.ascontiguousarray(feed['ph_lin_specs'], dtype=np.float32).reshape(B, -1, F)
    T = target.shape[1]
    min_frames = hp.n_fft // 2 // hop + 2            # the smallest n with hop (n - 1) > n_fft / 2
    if T < min_frames:
        return None
    tracks = []
    for lin, n in ((out['linear'], n_pred), (target, n_target)):
        frames = np.minimum(T, np.maximum(min_frames, np.asarray(n, np.int32))).astype(np.int32)
        mag = eng.denorm_power(lin, loader.mel_mag_ref_db, loader.mel_mag_max_db, hp.magnitude_power)
        wav, _ = eng.griffin_lim(mag, hp.reconstruction_iterations if f0_iters is None else f0_iters, win_len, hop, hp.n_fft,
                                 seed=seed, want_mse=False, momentum=0.0, n_frames=frames)
        tracks.append(eng.f0(wav, hp.sampling_rate, hop, fmin=f0_min, fmax=f0_max, n_samples=hop * (frames - 1)))
        mag.free()
        wav.free()
    res = f0_errors(tracks[0], tracks[1], path, engine=eng)
    for t in tracks:
        t.free()
    return res


def batch_stoi(model, feed, extended=False, stoi_iters=None, seed=0, want_wavs=False):
    """STOI (``extended``: ESTOI) of every utterance of one batch: ONE teacher-forced pass (``teacher_forced_device`` with
    ``want_linear``), then the predicted and the target linear spectrograms both become waveforms through the same ragged
    Griffin-Lim -- the same seed and the same frame counts, ``ph_time_frames * r`` -- and ``audio.metrics.stoi`` measures the
    prediction's against the target's.  -> (B,) float64 (NaN: fewer than 30 frames within 40 dB of the target's loudest), or None
    where the batch is shorter than the vocoder's shortest signal; with ``want_wavs`` also (the target's waveforms, the
    prediction's, their lengths), host arrays."""
    from ..audio.metrics import stoi
    from ..audio.conversion import ms_to_samples
    eng, hp = model.engine, model.hparams
    loader = dataset_params.dataset_loader
    win_len, hop = ms_to_samples(hp.win_len, hp.sampling_rate), ms_to_samples(hp.win_hop, hp.sampling_rate)
    B = feed['ph_sentences'].shape[0]
    F = 1 + hp.n_fft // 2
    target = np.ascontiguousarray(feed['ph_lin_specs'], dtype=np.float32).reshape(B, -1, F)
    T = target.shape[1]
    min_frames = hp.n_fft // 2 // hop + 2            # the smallest n with hop (n - 1) > n_fft / 2
    if T < min_frames:
        return None
    out = model.teacher_forced_device(feed['ph_sentences'], feed['ph_mel_specs'], None, want_mel=False, want_alignments=False,
                                      want_linear=True)
    n = np.asarray(feed['ph_time_frames'], np.int32) * eng.cfg.reduction
    frames = np.minimum(T, np.maximum(min_frames, n)).astype(np.int32)
    lens = (hop * (frames - 1)).astype(np.int32)
    wavs = []
    for lin in (target, out['linear']):
        mag = eng.denorm_power(lin, loader.mel_mag_ref_db, loader.mel_mag_max_db, hp.magnitude_power)
        wav, _ = eng.griffin_lim(mag, hp.reconstruction_iterations if stoi_iters is None else stoi_iters, win_len, hop, hp.n_fft,
                                 seed=seed, want_mse=False, momentum=0.0, n_frames=frames)
        wavs.append(wav.to_host()[:, :int(lens.max())].copy())
        mag.free()
        wav.free()
    for a in out.values():
        if hasattr(a, 'free'):
            a.free()
    values = stoi(wavs[0], wavs[1], hp.sampling_rate, extended=extended, n_samples=lens, engine=eng)
    return (values, wavs[0], wavs[1], lens) if want_wavs else values


def evaluate(model, checkpoint_file, batches, checkpoint_dir=None, checkpoint_save_run=None, verbose=True, mcd=False, mcd_coeffs=13,
             mcd_stop_at_silence=None, f0=False, f0_iters=None, f0_min=60.0, f0_max=500.0, attention=False, stoi=False, estoi=False,
             stoi_iters=None):
    """reference :153-257.  Restores ``checkpoint_file`` into ``model`` (a ``Tacotron(..., Mode.EVAL)``) once, runs every
    feed dict of ``batches`` through tts_evaluate and returns ``{loss, loss_decoder, loss_post_processing, global_step,
    n_batches}``: the per-batch float32 losses averaged unweighted over the batches.  Raises if no batch ran.  Appends
    the summary line (module docstring) when ``checkpoint_dir`` (default ``evaluation_params.checkpoint_dir``) is set.
    With ``mcd`` the result gains ``mcd`` -- the mean mel-cepstral distortion over all utterances of the epoch, in dB -- and
    ``mcd_utterances``, and the summary line ``metric/mcd``; without it nothing of the run, the result or the line changes.
    With ``f0`` the result and the summary line gain ``metric/f0_rmse_cents``, ``metric/f0_rmse_hz``, ``metric/vuv_error`` and
    ``metric/gross_pitch_error`` -- each the mean over the utterances that have that figure -- and ``f0_utterances``, the
    utterances that have an F0 RMSE (``f0_iters``: Griffin-Lim iterations, default the model's ``reconstruction_iterations``;
    ``f0_min`` / ``f0_max``: the search range in Hz); without it nothing of the run, the result or the line changes.
    With ``attention`` the result and the summary line gain ``attention/<flag>`` for every flag of
    ``attention_check.FLAGS`` -- the utterances of the epoch that carry it -- ``attention/mean_focus``, the mean over the
    utterances of focus_sum / n_steps, and ``attention_utterances``: ``Engine.alignment_stats`` on every batch's alignments, with
    the batch's own sentence lengths and frame counts; without it nothing of the run, the result or the line changes.
    With ``stoi`` the result and the summary line gain ``metric/stoi`` -- with ``estoi`` ``metric/estoi`` instead -- the mean of
    :func:`batch_stoi` over the utterances with a finite figure (NaN when there is none), and ``stoi_utterances``, their count
    (``stoi_iters``: Griffin-Lim iterations, default the model's ``reconstruction_iterations``); without it nothing of the run,
    the result or the line changes."""
    if estoi and not stoi:
        raise ValueError('evaluate: estoi needs stoi')
    if model._mode != Mode.EVAL:
        raise ValueError('evaluate() needs a Tacotron in Mode.EVAL')
    global_step = global_step_of(checkpoint_file)
    if verbose:
        print('[checkpoint_file] step: {}, file: "{}"'.format(global_step, checkpoint_file))
        print('Restoring model...')
    model.restore(checkpoint_file)
    if verbose:
        print('Restoring finished')
    sums = np.zeros(3, np.float64)
    n_batches = 0
    mcds = []
    f0s = []
    stois = []
    records = []
    for feed in batches:
        out = model.evaluate_device(feed['ph_sentences'], feed['ph_mel_specs'], feed['ph_lin_specs'],
                                    want_mel=bool(mcd) or bool(f0), want_alignments=bool(attention),
                                    want_linear=(bool(mcd) and mcd_stop_at_silence is not None) or bool(f0))
        sums += out['losses'].to_host().astype(np.float64)
        if attention:
            records.append(model.engine.alignment_stats(out['alignments'], n_sent=feed['ph_sentence_length'],
                                                        n_steps=feed['ph_time_frames']))
        if f0:
            res, n_pred, n_target = batch_alignment(model, feed, out, mcd_coeffs, mcd_stop_at_silence, want_path=True)
            if mcd:
                mcds.append(res['mcd'])
            errs = batch_f0(model, feed, out, res['path'], n_pred, n_target, f0_iters, f0_min, f0_max)
            if errs is not None:
                f0s.append(errs)
        elif mcd:
            mcds.append(batch_mcd(model, feed, out, mcd_coeffs, mcd_stop_at_silence))
        if stoi:
            values = batch_stoi(model, feed, extended=bool(estoi), stoi_iters=stoi_iters)
            if values is not None:
                stois.append(values)
        n_batches += 1
    if n_batches == 0:
        raise Exception('Error: No batches were processed!')
    avg = sums / n_batches
    result = dict(loss=float(avg[0]), loss_decoder=float(avg[1]), loss_post_processing=float(avg[2]),
                  global_step=global_step, n_batches=n_batches)
    if mcd:
        per_utterance = np.concatenate(mcds).astype(np.float64)
        result['mcd'] = float(np.mean(per_utterance))
        result['mcd_utterances'] = int(per_utterance.shape[0])
    if f0:
        for key in F0_KEYS:
            values = np.concatenate([e[key] for e in f0s]) if f0s else np.zeros(0)
            values = values[np.isfinite(values)]
            result['metric/' + key] = float(np.mean(values)) if values.size else float('nan')
            if key == 'f0_rmse_cents':
                result['f0_utterances'] = int(values.size)
    stoi_key = 'metric/estoi' if estoi else 'metric/stoi'
    if stoi:
        values = np.concatenate(stois) if stois else np.zeros(0)
        values = values[np.isfinite(values)]
        result[stoi_key] = float(np.mean(values)) if values.size else float('nan')
        result['stoi_utterances'] = int(values.size)
    if attention:
        from . import attention_check
        every = np.concatenate(records)
        verdicts = attention_check.verdict(every)
        for flag in attention_check.FLAGS:
            result['attention/' + flag] = int(sum(flag in v for v in verdicts))
        result['attention/mean_focus'] = float(np.mean(every['focus_sum'] / every['n_steps']))
        result['attention_utterances'] = int(every.shape[0])
    if verbose:
        print('[evaluate] step: {}, batches: {}, loss: {:.6f}, loss_decoder: {:.6f}, loss_post_processing: {:.6f}'.format(
            global_step, n_batches, result['loss'], result['loss_decoder'], result['loss_post_processing']))
        if mcd:
            print('[evaluate] step: {}, utterances: {}, mcd: {:.6f} dB'.format(global_step, result['mcd_utterances'], result['mcd']))
        if f0:
            print('[evaluate] step: {}, utterances: {}, f0_rmse: {:.3f} cents / {:.3f} Hz, vuv_error: {:.4f}, gross_pitch_error: {:.4f}'.format(
                global_step, result['f0_utterances'], *(result['metric/' + key] for key in F0_KEYS)))
        if stoi:
            print('[evaluate] step: {}, utterances: {}, {}: {:.6f}'.format(global_step, result['stoi_utterances'], stoi_key[7:], result[stoi_key]))
    checkpoint_dir = evaluation_params.checkpoint_dir if checkpoint_dir is None else checkpoint_dir
    if checkpoint_dir:
        save_dir = os.path.join(checkpoint_dir, checkpoint_save_run or evaluation_params.checkpoint_save_run)
        os.makedirs(save_dir, exist_ok=True)
        line = {'global_step': global_step, 'checkpoint': checkpoint_file, 'n_batches': n_batches,
                'loss/loss': result['loss'], 'loss/loss_decoder': result['loss_decoder'],
                'loss/loss_post_processing': result['loss_post_processing']}
        if mcd:
            line['metric/mcd'] = result['mcd']
        if f0:
            for key in F0_KEYS:
                line['metric/' + key] = result['metric/' + key]
            line['f0_utterances'] = result['f0_utterances']
        if stoi:
            line[stoi_key] = result[stoi_key]
            line['stoi_utterances'] = result['stoi_utterances']
        if attention:
            for key in sorted(k for k in result if k.startswith('attention')):
                line[key] = result[key]
        with open(os.path.join(save_dir, SUMMARY_FILE), 'a') as f:
            f.write(json.dumps(line) + '\n')
    return result


def collect_checkpoint_paths(checkpoint_dir):
    """reference :284-326: the ``all_model_checkpoint_paths`` entries of ``<checkpoint_dir>/checkpoint`` (the first line,
    ``model_checkpoint_path``, is dropped), joined onto the directory."""
    with open(os.path.join(checkpoint_dir, 'checkpoint'), 'r') as f:
        lines = [line.strip() for line in f]
    lines = lines[1:]
    lines = [line.replace('all_model_checkpoint_paths: ', '') for line in lines]
    lines = [line.replace('"', '') for line in lines]
    return [os.path.join(checkpoint_dir, line) for line in lines]


def evaluate_checkpoint(checkpoint_file, dataset_folder=None, max_samples=None, batch_size=None, checkpoint_dir=None,
                        checkpoint_save_run=None, hparams=None, device_id=0, verbose=True, mcd=False, mcd_coeffs=13,
                        mcd_stop_at_silence=None, f0=False, f0_iters=None, f0_min=60.0, f0_max=500.0, attention=False, stoi=False,
                        estoi=False, stoi_iters=None):
    """One cycle of the reference's ``__eval_cycle`` (:336-352): a dataset loader, the batches, a model with its own
    engine, :func:`evaluate`; the engine is released afterwards."""
    from ..datasets.lj_speech import LJSpeechDatasetHelper
    dataset = LJSpeechDatasetHelper(dataset_folder=dataset_folder or dataset_params.dataset_folder,
                                    char_dict=dataset_params.vocabulary_dict, fill_dict=False)
    batches = batched_placeholders(dataset,
                                   evaluation_params.max_samples if max_samples is None else max_samples,
                                   evaluation_params.batch_size if batch_size is None else batch_size, verbose=verbose)
    model = Tacotron(Tacotron.model_placeholders(), Mode.EVAL, hparams=hparams or model_params, device_id=device_id)
    try:
        return evaluate(model, checkpoint_file, batches, checkpoint_dir=checkpoint_dir,
                        checkpoint_save_run=checkpoint_save_run, verbose=verbose, mcd=mcd, mcd_coeffs=mcd_coeffs,
                        mcd_stop_at_silence=mcd_stop_at_silence, f0=f0, f0_iters=f0_iters, f0_min=f0_min, f0_max=f0_max,
                        attention=attention, stoi=stoi, estoi=estoi, stoi_iters=stoi_iters)
    finally:
        model.engine.close()


def main(argv=None):
    """The reference's ``python tacotron/evaluate.py`` (:329-364):

        python -m single-speaker-tts_amd.tacotron.evaluate [--all] [--checkpoint-dir D] [--load-run R] [--save-run S]
                                                           [--dataset-folder F] [--max-samples N] [--batch-size B]
                                                           [--mcd [--mcd-coeffs K] [--mcd-stop-at-silence DB]]
                                                           [--f0 [--f0-iters N] [--f0-min HZ] [--f0-max HZ]]
                                                           [--attention] [--stoi [--estoi] [--stoi-iters N]]

    The options override the ``evaluation_params`` / ``dataset_params`` fields of the same name.  Without ``--all``
    (``evaluate_all_checkpoints``) the latest checkpoint of ``<checkpoint_dir>/<load_run>`` is evaluated, with it every
    checkpoint its listing file names.  ``--mcd`` adds the mel-cepstral distortion, ``--f0`` the F0 RMSE, voicing error
    and gross pitch error along the same alignment, ``--stoi`` the intelligibility of the teacher-forced prediction against its
    target (module docstring).  Prints one JSON line per checkpoint."""
    import argparse
    from .checkpoint import latest_checkpoint
    ap = argparse.ArgumentParser(prog='tacotron.evaluate')
    ap.add_argument('--all', action='store_true', default=evaluation_params.evaluate_all_checkpoints)
    ap.add_argument('--checkpoint-dir', default=evaluation_params.checkpoint_dir)
    ap.add_argument('--load-run', default=evaluation_params.checkpoint_load_run)
    ap.add_argument('--save-run', default=evaluation_params.checkpoint_save_run)
    ap.add_argument('--dataset-folder', default=dataset_params.dataset_folder)
    ap.add_argument('--max-samples', type=int, default=evaluation_params.max_samples)
    ap.add_argument('--batch-size', type=int, default=evaluation_params.batch_size)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--mcd', action='store_true', help='also report the DTW-aligned mel-cepstral distortion in dB')
    ap.add_argument('--mcd-coeffs', type=int, default=13, help='cepstral coefficients 1 .. K are compared (default 13)')
    ap.add_argument('--mcd-stop-at-silence', type=float, default=None, metavar='DB',
                    help='end every prediction behind its last linear frame above DB decibels')
    ap.add_argument('--f0', action='store_true', help='also report F0 RMSE, voicing error and gross pitch error along the DTW path')
    ap.add_argument('--f0-iters', type=int, default=None, metavar='N',
                    help="Griffin-Lim iterations of --f0 (default: the model's reconstruction_iterations)")
    ap.add_argument('--f0-min', type=float, default=None, metavar='HZ', help='lowest F0 searched (default 60)')
    ap.add_argument('--f0-max', type=float, default=None, metavar='HZ', help='highest F0 searched (default 500)')
    ap.add_argument('--attention', action='store_true',
                    help='also report the attention diagnostics: utterances per flag of tacotron.attention_check, and the mean focus')
    ap.add_argument('--stoi', action='store_true',
                    help="also report the STOI of the teacher-forced prediction's waveform against the target's")
    ap.add_argument('--estoi', action='store_true', help='with --stoi: the extended form (ESTOI)')
    ap.add_argument('--stoi-iters', type=int, default=None, metavar='N',
                    help="Griffin-Lim iterations of --stoi (default: the model's reconstruction_iterations)")
    args = ap.parse_args(argv)
    if not args.stoi and (args.estoi or args.stoi_iters is not None):
        ap.error('--estoi and --stoi-iters need --stoi')
    if args.stoi_iters is not None and args.stoi_iters < 0:
        ap.error('--stoi-iters must be >= 0')
    if not args.f0 and (args.f0_iters is not None or args.f0_min is not None or args.f0_max is not None):
        ap.error('--f0-iters, --f0-min and --f0-max need --f0')
    if args.f0_iters is not None and args.f0_iters < 0:
        ap.error('--f0-iters must be >= 0')
    f0_min, f0_max = 60.0 if args.f0_min is None else args.f0_min, 500.0 if args.f0_max is None else args.f0_max
    if args.f0 and not 0 < f0_min <= f0_max:
        ap.error('need 0 < --f0-min <= --f0-max')
    if not args.mcd and (args.mcd_coeffs != 13 or args.mcd_stop_at_silence is not None):
        ap.error('--mcd-coeffs and --mcd-stop-at-silence need --mcd')
    load_dir = os.path.join(args.checkpoint_dir, args.load_run)
    if args.all:
        files = collect_checkpoint_paths(load_dir)
        print('Found #{} checkpoints to evalue.'.format(len(files)))
    else:
        latest = latest_checkpoint(load_dir)
        if latest is None:
            raise FileNotFoundError('no checkpoint found in {}'.format(load_dir))
        files = [latest]
    for checkpoint_file in files:
        res = evaluate_checkpoint(checkpoint_file, dataset_folder=args.dataset_folder, max_samples=args.max_samples,
                                  batch_size=args.batch_size, checkpoint_dir=args.checkpoint_dir,
                                  checkpoint_save_run=args.save_run, device_id=args.device, mcd=args.mcd,
                                  mcd_coeffs=args.mcd_coeffs, mcd_stop_at_silence=args.mcd_stop_at_silence, f0=args.f0,
                                  f0_iters=args.f0_iters, f0_min=f0_min, f0_max=f0_max, attention=args.attention,
                                  stoi=args.stoi, estoi=args.estoi, stoi_iters=args.stoi_iters)
        print(json.dumps(dict(res, checkpoint=checkpoint_file)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
