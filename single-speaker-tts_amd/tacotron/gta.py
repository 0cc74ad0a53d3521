"""Ground-truth-aligned (GTA) spectrograms of a recorded corpus: the network of a trained checkpoint run with teacher forcing
(reference tacotron/helpers.py:208-405, TacotronTrainingHelper; ``Tacotron.teacher_forced_device``) over the evaluation
batches, one ``.npz`` per utterance.

    python -m single-speaker-tts_amd.tacotron.gta [--dataset-folder D] [--checkpoint P] [--out-dir O] [--batch-size N]
                                                  [--max-samples N] [--linear] [--wav [--gl-iters N]] [--attention]

The decoder reads the GO frame at step 0 and frame t*r - 1 of the recording's pre-computed mel features at step t >= 1;
its predicted frames therefore line up with the recording (the usual training input of a neural vocoder).  The network is
the inference one otherwise -- no dropout, batch norm from the moving statistics, no gradient: this is not Mode.TRAIN.

Batches come from ``evaluate.batched_placeholders`` (its fixed order and padding).  As in the reference's training, the
attention has no mask: an utterance's outputs depend on the padding of its batch (T_sent, T_red), not on the batch size or
its position in the batch.  Every utterance gets ``<out-dir>/<wav stem>.gta.npz``, cropped to its own frame count T_red and
sentence length T_sent (with EOS):

* ``mel_mag_db`` (T_red, n_mels*r): the key and layout of the pre-computed features (``DatasetHelper.load_features``);
* ``alignments`` (T_red, T_sent);
* ``durations`` (T_sent,) int32: r x the number of decoder steps whose alignment argmax, over the utterance's own
  positions, is that position (they sum to T_red * r);
* with ``--attention``, ``attention_stats``: the utterance's alignment record (``Engine.alignment_stats`` on the batch, its own T_red steps and T_sent
  positions; ``_hip.ALIGNMENT_RECORD``, shape ()) -- what ``tacotron.attention_check.verdict`` reads; its durations, times r,
  are ``durations``;
* with ``--linear``, ``linear_mag_db`` (T_red, F*r).

``--wav`` also writes ``<out-dir>/<wav stem>.gta.wav``: the linear GTA spectrograms of a batch through one
``tts_denorm_power`` and ONE ragged Griffin-Lim call (``Engine.griffin_lim(n_frames=...)``), every utterance reconstructed
from its own T_red * r frames alone (the padding of its batch does not reach its waveform), ``--gl-iters`` iterations
(default: the model's ``reconstruction_iterations``), peak-normalised float32 like the synthesis entry point's files.

Prints one JSON line: the teacher-forced L1 losses (reference tacotron/model.py:432-442) averaged unweighted over the
batches, and the number of files written."""
import json
import os

import numpy as np

from . import evaluate as E
from ..audio.conversion import ms_to_samples
from ..audio.io import save_wav
from .model import Mode, Tacotron
from .params import dataset_params, evaluation_params, model_params

SUFFIX = '.gta.npz'
WAV_SUFFIX = '.gta.wav'


def gta_path(out_dir, wav_path):
    """``<out_dir>/<stem of wav_path>.gta.npz``"""
    return os.path.join(out_dir, os.path.splitext(os.path.basename(wav_path))[0] + SUFFIX)


def durations(alignments, reduction):
    """alignments (T_red, T_sent) of one utterance, already cropped -> (T_sent,) int32: reduction x the number of steps
    whose argmax is that position (the first maximum on ties)."""
    n_sent = alignments.shape[1]
    return (np.bincount(np.argmax(alignments, axis=1), minlength=n_sent) * reduction).astype(np.int32)


def crop(mel, alignments, linear, b, n_frames, n_sent, reduction):
    """Utterance b of a batch's host outputs -- mel (B, T, n_mels), alignments (T_red, B, T_sent), linear (B, T, F) or
    None -- cropped to its own n_frames decoder steps and n_sent positions: the arrays of its ``.gta.npz``."""
    B = mel.shape[0]
    out = dict(mel_mag_db=np.ascontiguousarray(mel.reshape(B, -1, reduction * mel.shape[2])[b, :n_frames]),
               alignments=np.ascontiguousarray(alignments[:n_frames, b, :n_sent]))
    out['durations'] = durations(out['alignments'], reduction)
    if linear is not None:
        out['linear_mag_db'] = np.ascontiguousarray(linear.reshape(B, -1, reduction * linear.shape[2])[b, :n_frames])
    return out


def gta_waveforms(model, linear, time_frames, n_iter=None, seed=0):
    """linear: the (B, T, F) device array of a teacher-forced batch; time_frames: T_red of every utterance.  One
    tts_denorm_power and one ragged Griffin-Lim call; returns B float32 arrays of hop (T_red r - 1) samples."""
    hp = model.hparams
    loader = dataset_params.dataset_loader
    win_len = ms_to_samples(hp.win_len, hp.sampling_rate)
    win_hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    frames = [int(t) * hp.reduction for t in time_frames]
    mag = model.engine.denorm_power(linear, loader.mel_mag_ref_db, loader.mel_mag_max_db, hp.magnitude_power)
    wav, _ = model.engine.griffin_lim(mag, hp.reconstruction_iterations if n_iter is None else n_iter, win_len, win_hop,
                                      hp.n_fft, seed=seed, want_mse=False, momentum=0.0, n_frames=frames)
    wav = wav.to_host()
    return [wav[b, :win_hop * (n - 1)].copy() for b, n in enumerate(frames)]


def write_gta(model, batches, out_dir, with_linear=False, verbose=True, with_wav=False, gl_iters=None, seed=0, attention_stats=False):
    """batches: (feed dict of ``evaluate.batched_placeholders``, wav paths of its utterances) pairs.  Runs every batch
    through ``model.teacher_forced_device`` (a Tacotron, or anything with that method), writes the ``.gta.npz`` files (with
    ``with_wav`` the ``.gta.wav`` files as well: ``gta_waveforms``, which needs ``model.engine``; with ``attention_stats`` every
    ``.gta.npz`` also carries its utterance's alignment record, which needs ``model.engine`` too) and returns
    ``{loss, loss_decoder, loss_post_processing, n_batches, n_files}``."""
    os.makedirs(out_dir, exist_ok=True)
    r = model.hparams.reduction
    sums = np.zeros(3, np.float64)
    n_batches = n_files = 0
    for feed, wav_paths in batches:
        out = model.teacher_forced_device(feed['ph_sentences'], feed['ph_mel_specs'], feed['ph_lin_specs'],
                                          want_mel=True, want_alignments=True, want_linear=with_linear or with_wav)
        mel, al = out['mel'].to_host(), out['alignments'].to_host()
        # the alignment records of the batch, from the alignments where they lie
        records = model.engine.alignment_stats(out['alignments'], n_sent=feed['ph_sentence_length'],
                                               n_steps=feed['ph_time_frames']) if attention_stats else None
        lin = out['linear'].to_host() if with_linear else None
        sums += out['losses'].to_host().astype(np.float64)
        wavs = gta_waveforms(model, out['linear'], feed['ph_time_frames'][:len(wav_paths)], gl_iters, seed + n_batches) if with_wav else None
        n_batches += 1
        for b, wav_path in enumerate(wav_paths):
            arrays = crop(mel, al, lin, b, int(feed['ph_time_frames'][b]), int(feed['ph_sentence_length'][b]), r)
            if records is not None:
                arrays['attention_stats'] = records[b]
            np.savez(gta_path(out_dir, wav_path), **arrays)
            if with_wav:
                save_wav(gta_path(out_dir, wav_path)[:-len(SUFFIX)] + WAV_SUFFIX, wavs[b], model.hparams.sampling_rate, True,
                         engine=model.engine)
            n_files += 1
    if n_batches == 0:
        raise Exception('Error: No batches were processed!')
    avg = sums / n_batches
    result = dict(loss=float(avg[0]), loss_decoder=float(avg[1]), loss_post_processing=float(avg[2]), n_batches=n_batches,
                  n_files=n_files)
    if verbose:
        print('[gta] batches: {}, files: {}, loss: {:.6f}, loss_decoder: {:.6f}, loss_post_processing: {:.6f}'.format(
            n_batches, n_files, result['loss'], result['loss_decoder'], result['loss_post_processing']))
    return result


class _Recording(object):
    """A dataset helper that keeps what its ``load`` returned (the wav paths of the batches)."""

    def __init__(self, dataset):
        self.dataset = dataset
        self.loaded = None

    def load(self, max_samples=None):
        self.loaded = self.dataset.load(max_samples=max_samples)
        return self.loaded

    def load_audio(self, wav_path):
        return self.dataset.load_audio(wav_path)


def batches_with_paths(dataset, max_samples, batch_size, verbose=True):
    """``evaluate.batched_placeholders`` with the wav paths of every batch's utterances, from the same bucketing."""
    rec = _Recording(dataset)
    n_buckets, allow = evaluation_params.n_buckets, evaluation_params.allow_smaller_batches
    feeds = E.batched_placeholders(rec, max_samples, batch_size, n_buckets=n_buckets, allow_smaller_batches=allow,
                                   verbose=verbose)
    order = None
    for k, feed in enumerate(feeds):
        if order is None:   # (the generator has loaded the listing by now)
            _, lengths, wav_paths = rec.loaded
            order = [[wav_paths[i] for i in idx]
                     for idx in E.bucket_batches(lengths, E.bucket_boundaries(lengths, n_buckets), batch_size, allow)]
        yield feed, order[k]


def main(argv=None):
    import argparse
    from .checkpoint import latest_checkpoint
    ap = argparse.ArgumentParser(prog='tacotron.gta', description='teacher-forced (ground-truth-aligned) spectrograms')
    ap.add_argument('--dataset-folder', default=dataset_params.dataset_folder)
    ap.add_argument('--checkpoint', default=None,
                    help='checkpoint prefix, run directory or .npz (default: the latest of the evaluation run)')
    ap.add_argument('--out-dir', default=None, help='default: <dataset-folder>/gta')
    ap.add_argument('--batch-size', type=int, default=evaluation_params.batch_size)
    ap.add_argument('--max-samples', type=int, default=evaluation_params.max_samples)
    ap.add_argument('--linear', action='store_true', help='also write linear_mag_db')
    ap.add_argument('--wav', action='store_true', help='also write <stem>.gta.wav (one ragged Griffin-Lim call per batch)')
    ap.add_argument('--gl-iters', type=int, default=None, metavar='N',
                    help="Griffin-Lim iterations of --wav (default: the model's reconstruction_iterations)")
    ap.add_argument('--attention', action='store_true',
                    help='also write attention_stats, the alignment record of tacotron.attention_check, into every .gta.npz')
    ap.add_argument('--device', type=int, default=0)
    args = ap.parse_args(argv)
    if args.gl_iters is not None and (not args.wav or args.gl_iters < 0):
        ap.error('--gl-iters: a count of iterations, with --wav')
    checkpoint = args.checkpoint
    if checkpoint is None:
        load_dir = os.path.join(evaluation_params.checkpoint_dir, evaluation_params.checkpoint_load_run)
        checkpoint = latest_checkpoint(load_dir)
        if checkpoint is None:
            raise FileNotFoundError('no checkpoint found in {}'.format(load_dir))
    from ..datasets.lj_speech import LJSpeechDatasetHelper
    dataset = LJSpeechDatasetHelper(dataset_folder=args.dataset_folder, char_dict=dataset_params.vocabulary_dict,
                                    fill_dict=False)
    model = Tacotron(Tacotron.model_placeholders(), Mode.PREDICT, hparams=model_params, device_id=args.device)
    try:
        model.restore(checkpoint)
        res = write_gta(model, batches_with_paths(dataset, args.max_samples, args.batch_size),
                        args.out_dir or os.path.join(args.dataset_folder, 'gta'), with_linear=args.linear,
                        with_wav=args.wav, gl_iters=args.gl_iters, attention_stats=args.attention)
    finally:
        model.engine.close()
    print(json.dumps(dict(res, checkpoint=checkpoint)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
