"""Mirror of the reference's ``tacotron/dataset_statistics.py``: the vocabulary of a dataset's transcripts and the four dB
constants of the feature normalisation (datasets.statistics.collect_decibel_statistics), printed under the reference's
names -- which it crosses: the mean max mel dB is printed as ``mel_mag_ref_db``, the mean min as ``mel_mag_max_db``, and
likewise for the linear constants.

    python -m single-speaker-tts_amd.tacotron.dataset_statistics [--dataset-folder DIR] [--reconstruction-iters N] [--loudness]
                                                                  [--reconstruction-stoi N [--estoi]]

``--reconstruction-iters N`` adds the reference's Griffin-Lim reconstruction error after N iterations
(datasets.statistics.collect_reconstruction_error) behind the dB statistics; ``--loudness`` adds the corpus's integrated
loudness after ITU-R BS.1770-4 (datasets.statistics.collect_loudness: min / max / mean / standard deviation in LUFS) behind
those; ``--reconstruction-stoi N`` adds the intelligibility (STOI, with ``--estoi`` ESTOI) of every recording's Griffin-Lim
reconstruction after N iterations against the recording (datasets.statistics.collect_intelligibility) behind those.  Without the
switches the output is what it was."""
import argparse
import os

from ..datasets.lj_speech import LJSpeechDatasetHelper
from ..datasets.statistics import collect_decibel_statistics, collect_intelligibility, collect_loudness, collect_reconstruction_error
from .params import dataset_params


def main(argv=None):
    ap = argparse.ArgumentParser(prog='tacotron.dataset_statistics')
    ap.add_argument('--dataset-folder', default=dataset_params.dataset_folder)
    ap.add_argument('--reconstruction-iters', type=int, default=None, metavar='N',
                    help='also print the mean Griffin-Lim reconstruction error after N iterations')
    ap.add_argument('--loudness', action='store_true',
                    help='also print the integrated loudness (ITU-R BS.1770-4) of the recordings: min / max / mean / std in LUFS')
    ap.add_argument('--reconstruction-stoi', type=int, default=None, metavar='N',
                    help="also print the STOI of the recordings' Griffin-Lim reconstructions after N iterations: min / max / mean / std")
    ap.add_argument('--estoi', action='store_true', help='with --reconstruction-stoi: the extended form (ESTOI)')
    args = ap.parse_args(argv)
    if args.reconstruction_iters is not None and args.reconstruction_iters < 1:
        ap.error('--reconstruction-iters: at least one iteration')
    if args.reconstruction_stoi is not None and args.reconstruction_stoi < 1:
        ap.error('--reconstruction-stoi: at least one iteration')
    if args.estoi and args.reconstruction_stoi is None:
        ap.error('--estoi needs --reconstruction-stoi')
    dataset = LJSpeechDatasetHelper(dataset_folder=args.dataset_folder, char_dict={'pad': 0, 'eos': 1}, fill_dict=True)
    if not os.path.exists(args.dataset_folder):
        print("Dataset folder '{}' could not be found.".format(args.dataset_folder))
        return 1
    print('Dataset: {}'.format(args.dataset_folder))
    print('Loading dataset ...')
    _, _, paths = dataset.load()
    print('Dataset vocabulary:')
    sorted_by_value = sorted(dataset._char2idx_dict.items(), key=lambda kv: kv[1])
    print('vocabulary_dict={')
    for k, v in sorted_by_value:
        print("    '{}': {},".format(k, v))
    print('},')
    print('vocabulary_size={}'.format(len(sorted_by_value)))
    print('\n\n')
    print('Collecting decibel statistics for {} files ...'.format(len(paths)))
    min_linear_db, max_linear_db, min_mel_db, max_mel_db = collect_decibel_statistics(paths)
    print('mel_mag_ref_db = ', max_mel_db)
    print('mel_mag_max_db = ', min_mel_db)
    print('linear_ref_db = ', max_linear_db)
    print('linear_mag_max_db = ', min_linear_db)
    if args.reconstruction_iters is not None:
        collect_reconstruction_error(paths, args.reconstruction_iters)
    if args.loudness:
        print('Collecting loudness statistics for {} files ...'.format(len(paths)))
        loud = collect_loudness(paths)
        print('loudness_lufs_min = ', loud['min'])
        print('loudness_lufs_max = ', loud['max'])
        print('loudness_lufs_mean = ', loud['mean'])
        print('loudness_lufs_std = ', loud['std'])
        print('loudness_measured = {} of {}'.format(loud['measured'], len(paths)))
    if args.reconstruction_stoi is not None:
        name = 'estoi' if args.estoi else 'stoi'
        print('Collecting reconstruction {} for {} files ...'.format(name, len(paths)))
        res = collect_intelligibility(paths, args.reconstruction_stoi, extended=args.estoi)
        for key in ('min', 'max', 'mean', 'std'):
            print('reconstruction_{}_{} = '.format(name, key), res[key])
        print('reconstruction_{}_measured = {} of {}'.format(name, res['measured'], len(paths)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
