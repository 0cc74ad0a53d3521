"""Mirror of the reference's ``tacotron/dataset_precalc_features.py``: write ``<wav stem>.npz`` features next to every
recording of the dataset (what ``tacotron.evaluate`` reads).

    python -m single-speaker-tts_amd.tacotron.dataset_precalc_features [--dataset-folder DIR] [--batch-size N]

``dataset_params.dataset_loader`` is only the constants class here; the loader is ``datasets.lj_speech.LJSpeechDatasetHelper``,
whose dB constants are the same."""
import argparse

from ..datasets.lj_speech import LJSpeechDatasetHelper
from .params import dataset_params


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='tacotron.dataset_precalc_features')
    ap.add_argument('--dataset-folder', default=dataset_params.dataset_folder)
    ap.add_argument('--batch-size', type=int, default=32, help='recordings per GPU feature batch')
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error('--batch-size must be >= 1')
    return args


def main(argv=None):
    args = parse_args(argv)
    dataset = LJSpeechDatasetHelper(dataset_folder=args.dataset_folder, char_dict=dict(dataset_params.vocabulary_dict),
                                    fill_dict=True)
    print('Dataset: {}'.format(args.dataset_folder))
    print('Loading dataset ...')
    _, _, paths = dataset.load()
    print('Pre-computing features for {} files ...'.format(len(paths)))
    dataset.pre_compute_features(paths, batch_size=args.batch_size)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
