"""LJ-Speech helper: dB constants, the abbreviation table and the corpus listing reader of reference
datasets/lj_speech.py (:20-29, :37-60, :62-103).  Evaluation reads audio features from the pre-computed ``.npz``
files (``DatasetHelper.load_features``); ``DatasetHelper.pre_compute_features`` writes them from the ``.wav`` files
as the reference's ``load_audio`` (:106-156) computes them, with these dB constants (features.hip on the GPU)."""
import csv
import os

from .dataset_helper import DatasetHelper


class LJSpeechDatasetHelper(DatasetHelper):
    mel_mag_ref_db = 6.02
    mel_mag_max_db = 99.89
    linear_ref_db = 35.66
    linear_mag_max_db = 100.0
    raw_silence_db = None

    def __init__(self, dataset_folder, char_dict, fill_dict):
        super().__init__(dataset_folder, char_dict, fill_dict)
        # order matters: str.replace is applied in insertion order and '.' -> '' must be last
        self._abbreviations = {
            'mr.': 'mister', 'mrs.': 'misses', 'dr.': 'doctor', 'no.': 'number', 'st.': 'saint',
            'co.': 'company', 'jr.': 'junior', 'maj.': 'major', 'gen.': 'general', 'drs.': 'doctors',
            'rev.': 'reverend', 'lt.': 'lieutenant', 'hon.': 'honorable', 'sgt.': 'sergeant',
            'capt.': 'captain', 'esq.': 'esquire', 'ltd.': 'limited', 'col.': 'colonel', 'ft.': 'fort',
            '[': '', ']': '', '.': '',
        }

    def load(self, max_samples=None, min_len=None, max_len=None, listing_file_name='metadata.csv'):
        """reference :62-103: ``<dataset>/<listing>`` rows ``id|transcript|normalised transcript`` ->
        (id_sequences (bytes of int32 arrays), sequence_lengths incl. EOS, ``<dataset>/wavs/<id>.wav`` paths).
        Sentences (ASCII, before lower-casing) shorter than ``min_len`` or longer than ``max_len`` are skipped;
        reading stops after ``max_samples`` kept rows."""
        data_file = os.path.join(self._dataset_folder, listing_file_name)
        wav_folder = os.path.join(self._dataset_folder, 'wavs')
        file_paths, sentences = [], []
        with open(data_file, 'r') as csv_file:
            for file_id, _, normalized_sentence in csv.reader(csv_file, delimiter='|', quotechar='|'):
                sentence = self.utf8_to_ascii(normalized_sentence)
                if min_len is not None and len(sentence) < min_len:
                    continue
                if max_len is not None and len(sentence) > max_len:
                    continue
                sentences.append(sentence)
                file_paths.append('{}.wav'.format(os.path.join(wav_folder, file_id)))
                if max_samples is not None and len(sentences) == max_samples:
                    break
        id_sentences, sentence_lengths = self.process_sentences(sentences)
        return id_sentences, sentence_lengths, file_paths
