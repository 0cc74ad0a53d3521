"""ctypes binding of libsstts_hip.so (the C ABI declared in include/sstts_hip.h).

This is the only compute path of the package: there is no CPU fallback.  If the shared
library is missing or a call fails, an exception is raised.

Host arrays are numpy; device memory is either owned by the library's allocator
(:class:`DeviceArray`) or borrowed from anything exposing ``data_ptr()`` (a CUDA/HIP torch
tensor) -- PyTorch is optional plumbing, not a dependency of this module.
"""
import collections
import contextlib
import ctypes
import math
import os
from ctypes import (POINTER, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64,
                    c_void_p)

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SSTTS_HIP_LIB') or os.path.join(_HERE, 'libsstts_hip.so')

TTS_OK = 0
TTS_ERR_INVALID = -1
TTS_ERR_NOT_LOADED = -2
TTS_ERR_HIP = -3
TTS_ERR_DB_RANGE = -4
TTS_ERR_UNSUPPORTED = -5


class TtsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('sstts_hip error {}: {}'.format(code, msg))
        self.code = code


class TtsConfig(ctypes.Structure):
    """struct tts_config (include/sstts_hip.h)."""
    _fields_ = [
        ('struct_size', c_int32),
        ('vocabulary_size', c_int32), ('embedding_size', c_int32), ('enc_prenet_units', c_int32 * 2),
        ('enc_n_banks', c_int32), ('enc_n_filters', c_int32), ('enc_proj_filters', c_int32 * 2),
        ('post_n_banks', c_int32), ('post_n_filters', c_int32), ('post_proj_filters', c_int32 * 2),
        ('n_highway_layers', c_int32), ('n_highway_units', c_int32), ('n_gru_units', c_int32),
        ('dec_prenet_units', c_int32 * 2), ('n_attention_units', c_int32),
        ('n_decoder_gru_units', c_int32), ('n_decoder_gru_layers', c_int32), ('n_mels', c_int32),
        ('reduction', c_int32), ('n_fft', c_int32), ('force_cudnn', c_int32),
        ('attention_mechanism', c_int32), ('luong_local_window_d', c_int32), ('luong_force_gaussian', c_int32),
        ('luong_local_mode', c_int32), ('apply_post_processing', c_int32),
    ]


class TtsSynthParams(ctypes.Structure):
    """struct tts_synth_params (include/sstts_hip.h)."""
    _fields_ = [
        ('n_steps', c_int32), ('ref_db', c_float), ('max_db', c_float), ('power', c_float),
        ('n_iter', c_int32), ('win_length', c_int32), ('hop_length', c_int32), ('seed', c_uint64),
        ('peak_normalize', c_int32), ('host_outputs', c_int32),
    ]


class TtsFeatureParams(ctypes.Structure):
    """struct tts_feature_params (include/sstts_hip.h)."""
    _fields_ = [
        ('struct_size', c_int32), ('n_fft', c_int32), ('win_length', c_int32), ('hop_length', c_int32),
        ('sampling_rate', c_int32), ('n_mels', c_int32), ('fmin', c_float), ('fmax', c_float),
        ('mel_ref_db', c_float), ('mel_max_db', c_float), ('linear_ref_db', c_float), ('linear_max_db', c_float),
        ('normalize', c_int32), ('reduction', c_int32), ('trim', c_int32), ('trim_top_db', c_float),
        ('trim_frame_length', c_int32), ('trim_hop_length', c_int32),
    ]


class TtsAlignmentStats(ctypes.Structure):
    """struct tts_alignment_stats (include/sstts_hip.h): twelve int32 and a double, 56 bytes."""
    _fields_ = [(name, c_int32) for name in ('n_sent', 'n_steps', 'reached', 'end_step', 'backward', 'max_back', 'max_jump',
                                             'longest_stall', 'after_end', 'off_text', 'skipped', 'reserved')] + [('focus_sum', ctypes.c_double)]


# ... and the same record as a numpy dtype: what Engine.alignment_stats returns an array of
ALIGNMENT_RECORD = np.dtype([(name, np.int32) for name, _t in TtsAlignmentStats._fields_[:12]] + [('focus_sum', np.float64)])


class TtsTokenTimesStats(ctypes.Structure):
    """struct tts_token_times_stats (include/sstts_hip.h): an int64 and six int32, 32 bytes."""
    _fields_ = [('score', c_int64)] + [(name, c_int32) for name in ('n_sent', 'n_steps', 'last', 'jumps', 'skipped', 'agree')]


# ... and the same record as a numpy dtype: what Engine.token_times returns an array of
TOKEN_TIMES_RECORD = np.dtype([('score', np.int64)] + [(name, np.int32) for name, _t in TtsTokenTimesStats._fields_[1:]])
TOKEN_TIMES_MAX_TOKENS = 1024    # tts_token_times_max_tokens()
TOKEN_TIMES_MAX_JUMP = 15        # the largest max_jump of tts_token_times


class TtsLimitStats(ctypes.Structure):
    """struct tts_limit_stats (include/sstts_hip.h): two int32 and a double, 16 bytes."""
    _fields_ = [('over', c_int32), ('limited', c_int32), ('min_gain', ctypes.c_double)]


# ... and the same record as a numpy dtype: what Engine.limit returns an array of
LIMIT_RECORD = np.dtype([('over', np.int32), ('limited', np.int32), ('min_gain', np.float64)])


class TtsEncodeStats(ctypes.Structure):
    """struct tts_encode_stats (include/sstts_hip.h): four int32, 16 bytes."""
    _fields_ = [('clipped', c_int32), ('nans', c_int32), ('peak', c_int32), ('n', c_int32)]


# ... and the same record as a numpy dtype: what Engine.encode and Engine.wait_host_encoded return an array of
ENCODE_RECORD = np.dtype([('clipped', np.int32), ('nans', np.int32), ('peak', np.int32), ('n', np.int32)])


class TtsJoinPiece(ctypes.Structure):
    """tts_join_piece_t: samples [first, first + count) of a row and the pause behind them; a row of the (P, 4) int32 arrays
    ``Engine.join`` hands the library"""
    _fields_ = [('row', c_int32), ('first', c_int32), ('count', c_int32), ('gap', c_int32)]


class TtsWarpSegment(ctypes.Structure):
    """tts_warp_segment_t: source frames [first, first + frames) of a row at ``step`` / 65536 source frames per output frame and a
    gain, or (frames == 0) a pause of ``pause`` output frames; 24 bytes, a record of the WARP_SEGMENT arrays ``Engine.warp_magnitudes``
    hands the library"""
    _fields_ = [('row', c_int32), ('first', c_int32), ('frames', c_int32), ('pause', c_int32), ('step', ctypes.c_uint32), ('gain', c_float)]


# ... and the same record as a numpy dtype
WARP_SEGMENT = np.dtype([('row', np.int32), ('first', np.int32), ('frames', np.int32), ('pause', np.int32), ('step', np.uint32), ('gain', np.float32)])


class TtsResampleSegment(ctypes.Structure):
    """tts_resample_segment_t: source samples [first, first + samples) of a row at ``ratio`` output samples per input sample
    (1.0 exactly: a copy); 24 bytes, a record of the RESAMPLE_SEGMENT arrays ``Engine.resample_segments`` hands the library"""
    _fields_ = [('row', c_int32), ('first', c_int32), ('samples', c_int32), ('reserved', c_int32), ('ratio', ctypes.c_double)]


# ... and the same record as a numpy dtype
RESAMPLE_SEGMENT = np.dtype([('row', np.int32), ('first', np.int32), ('samples', np.int32), ('reserved', np.int32), ('ratio', np.float64)])


class TtsShiftSegment(ctypes.Structure):
    """tts_shift_segment_t: the frames [first, first + frames) of a row with the fine structure read at ``pitch_step`` / 65536 and
    the envelope at ``formant_step`` / 65536 source bins per output bin; 24 bytes, a record of the SHIFT_SEGMENT arrays
    ``Engine.shift_magnitudes`` hands the library"""
    _fields_ = [('row', c_int32), ('first', c_int32), ('frames', c_int32), ('reserved', c_int32), ('pitch_step', ctypes.c_uint32),
                ('formant_step', ctypes.c_uint32)]


# ... and the same record as a numpy dtype
SHIFT_SEGMENT = np.dtype([('row', np.int32), ('first', np.int32), ('frames', np.int32), ('reserved', np.int32), ('pitch_step', np.uint32),
                          ('formant_step', np.uint32)])


_PROTOTYPES = {
    'tts_shift_plan': (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int]),
    'tts_shift_magnitudes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), c_void_p, c_int, c_int, c_void_p]),
    'tts_shift_max_segments': (c_int, []),
    'tts_shift_tile': (c_int, []),
    'tts_shift_max_order': (c_int, []),
    'tts_resample_segments_plan': (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int64)]),
    'tts_resample_segments': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_int, c_int, c_void_p, POINTER(c_int32)]),
    'tts_resample_segments_max': (c_int, []),
    'tts_resample_segments_max_ratios': (c_int, []),
    'tts_resample_segments_tile': (c_int, []),
    'tts_warp_plan': (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int64)]),
    'tts_warp_magnitudes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), c_void_p, c_int, c_int, c_void_p]),
    'tts_warp_max_segments': (c_int, []),
    'tts_warp_tile': (c_int, []),
    'tts_alignment_stats': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int32), c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    'tts_text_lengths': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tts_token_times': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int32), c_int, c_void_p, c_void_p,
                                c_void_p]),
    'tts_token_times_max_tokens': (c_int, []),
    'tts_set_token_times': (c_int, [c_void_p, c_int, c_int, c_int]),
    'tts_synth_token_times': (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    'tts_wait_host_token_times': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int), POINTER(c_int)]),
    'tts_set_alignment_stats': (c_int, [c_void_p, c_int, c_int]),
    'tts_synth_alignment_stats': (c_int, [c_void_p, c_void_p, c_int]),
    'tts_wait_host_alignment_stats': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int)]),
    'tts_speech_interval': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    'tts_join_plan': (c_int, [c_void_p, c_int, POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_int64)]),
    'tts_join': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, POINTER(c_int32), c_int, c_int, c_int, c_void_p]),
    'tts_join_max_pieces': (c_int, []),
    'tts_join_max_fade': (c_int, []),
    'tts_join_tile': (c_int, []),
    'tts_version': (c_char_p, []),
    'tts_default_config': (c_int, [POINTER(TtsConfig)]),
    'tts_create': (c_int, [POINTER(TtsConfig), c_int, POINTER(c_void_p)]),
    'tts_destroy': (c_int, [c_void_p]),
    'tts_last_error': (c_char_p, [c_void_p]),
    'tts_set_stream': (c_int, [c_void_p, c_void_p]),
    'tts_set_option': (c_int, [c_void_p, c_char_p, c_int]),
    'tts_synchronize': (c_int, [c_void_p]),
    'tts_manifest_size': (c_int, [c_void_p]),
    'tts_manifest_entry': (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int64), POINTER(c_int)]),
    'tts_set_weight': (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    'tts_load_weights_blob': (c_int, [c_void_p, c_void_p, c_size_t]),
    'tts_finalize_weights': (c_int, [c_void_p]),
    'tts_malloc': (c_int, [POINTER(c_void_p), c_size_t]),
    'tts_free': (c_int, [c_void_p]),
    'tts_device_malloc': (c_int, [c_void_p, POINTER(c_void_p), c_size_t]),
    'tts_device_free': (c_int, [c_void_p, c_void_p]),
    'tts_memcpy_h2d': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'tts_memcpy_d2h': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'tts_memset': (c_int, [c_void_p, c_void_p, c_int, c_size_t]),
    'tts_encoder_forward': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'tts_decoder_forward': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'tts_postnet_forward': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'tts_evaluate': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
    'tts_decoder_forward_teacher': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'tts_teacher_forced': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    'tts_teacher_kernel_choice': (c_int, [c_void_p, c_int, c_int]),
    'tts_denorm_power': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p]),
    'tts_griffin_lim': (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_void_p, c_void_p]),
    'tts_griffin_lim_ragged': (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_int, POINTER(c_int32), c_int, c_int,
                                       c_int, c_int, c_void_p, c_void_p]),
    'tts_peak_normalize': (c_int, [c_void_p, c_void_p, c_int, c_int]),
    'tts_speech_frames': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p]),
    'tts_speech_threshold': (c_int, [c_float, c_float, c_float, c_float, c_int, POINTER(c_float)]),
    'tts_set_end_of_speech': (c_int, [c_void_p, c_int, c_float, c_int]),
    'tts_synth_frames': (c_int, [c_void_p, POINTER(c_int32), c_int]),
    'tts_wait_host_frames': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int)]),
    'tts_stretched_frames': (c_int, [c_int, ctypes.c_double, POINTER(c_int)]),
    'tts_stretch_magnitudes': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), ctypes.c_double, c_int, c_void_p]),
    'tts_stretch_rows': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), ctypes.c_double, c_int, c_void_p]),
    'tts_set_speaking_rate': (c_int, [c_void_p, ctypes.c_double]),
    'tts_resampled_length': (c_int, [c_int, ctypes.c_double, POINTER(c_int)]),
    'tts_resample': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), ctypes.c_double, c_int, c_void_p]),
    'tts_set_pitch': (c_int, [c_void_p, ctypes.c_double]),
    'tts_phase_estimate': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_int, c_void_p]),
    'tts_phase_estimate_rows': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_int32), c_int, c_int, c_void_p]),
    'tts_phase_chunk_frames': (c_int, []),
    'tts_mfcc': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int, c_int, c_void_p]),
    'tts_dtw': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_int,
                        c_void_p, c_void_p, c_void_p]),
    'tts_dtw_max_frames': (c_int, []),
    'tts_dtw_tile': (c_int, []),
    'tts_f0': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), ctypes.c_double, c_int, c_int, c_int, c_int, ctypes.c_double,
                       c_void_p, c_void_p]),
    'tts_f0_frames': (c_int, [c_int, c_int]),
    'tts_f0_max_window': (c_int, []),
    'tts_f0_max_lag': (c_int, []),
    'tts_f0_compare': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'tts_loudness': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p]),
    'tts_loudness_normalize': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_int, ctypes.c_double, ctypes.c_double,
                                       c_void_p, c_void_p]),
    'tts_loudness_filter': (c_int, [c_int, POINTER(ctypes.c_double)]),
    'tts_loudness_segment': (c_int, [c_int]),
    'tts_set_loudness': (c_int, [c_void_p, c_int, ctypes.c_double, ctypes.c_double, c_int]),
    'tts_true_peak': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_void_p]),
    'tts_true_peak_filter': (c_int, [POINTER(ctypes.c_double)]),
    'tts_limit': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), ctypes.c_double, c_int, c_int, c_void_p]),
    'tts_limit_max_lookahead': (c_int, []),
    'tts_set_limiter': (c_int, [c_void_p, c_int, ctypes.c_double, c_int, c_int]),
    'tts_equalize': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), POINTER(ctypes.c_double), c_int]),
    'tts_equalizer_design': (c_int, [c_int, c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, POINTER(ctypes.c_double)]),
    'tts_equalizer_profile': (c_int, [c_char_p, c_int, POINTER(ctypes.c_double), POINTER(c_int)]),
    'tts_equalizer_max_sections': (c_int, []),
    'tts_set_equalizer': (c_int, [c_void_p, c_int, POINTER(ctypes.c_double), c_int]),
    'tts_compress': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_void_p, c_void_p]),
    'tts_compressor_design': (c_int, [c_int, ctypes.c_double, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    'tts_compressor_profile': (c_int, [c_char_p, c_int, c_void_p]),
    'tts_set_compressor': (c_int, [c_void_p, c_int, c_void_p]),
    'tts_watermark_embed': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_void_p]),
    'tts_watermark_detect': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tts_watermark_max_offsets': (c_int, []),
    'tts_stoi': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_void_p]),
    'tts_stoi_frames': (c_int, [c_int]),
    'tts_stoi_max_frames': (c_int, []),
    'tts_stoi_window': (c_int, [POINTER(ctypes.c_double)]),
    'tts_stoi_bands': (c_int, [POINTER(c_int32)]),
    'tts_set_watermark': (c_int, [c_void_p, c_int, c_void_p]),
    'tts_encode': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_int, ctypes.c_uint64, c_void_p, c_void_p]),
    'tts_encode_width': (c_int, [c_int]),
    'tts_encode_tile': (c_int, []),
    'tts_set_output': (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    'tts_wait_host_encoded': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_int), POINTER(c_int), POINTER(c_void_p),
                                      POINTER(c_void_p), POINTER(c_int)]),
    'tts_stft': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'tts_db_convert': (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_float, c_float, c_void_p]),
    'tts_stft_magnitude': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    'tts_mel_spectrogram': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                                    c_void_p]),
    'tts_trim_bounds': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    'tts_default_feature_params': (c_int, [POINTER(TtsFeatureParams)]),
    'tts_plan_features': (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(TtsFeatureParams), c_void_p]),
    'tts_extract_features': (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(TtsFeatureParams), c_void_p, c_void_p,
                                     c_void_p]),
    'tts_synthesize': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(TtsSynthParams), c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    'tts_synthesize_host': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(TtsSynthParams), POINTER(c_int)]),
    'tts_wait_host': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_size_t)]),
    'tts_wait_host_outputs': (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p), POINTER(c_size_t)]),
    'tts_profile_reset': (c_int, [c_void_p]),
    'tts_profile_get': (c_int, [c_void_p, c_char_p, POINTER(c_float), POINTER(c_int64)]),
    'tts_decoder_kernel_choice': (c_int, [c_void_p, c_int, c_int, c_int]),
    'tts_debug_workspace': (c_int, [c_void_p, c_char_p, POINTER(c_void_p), POINTER(c_size_t)]),
    'tts_debug_hold': (c_int, [c_void_p, c_int, c_int, ctypes.c_double]),
    'tts_debug_gemm': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    'tts_debug_gl_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int)]),
    'tts_debug_gl_plan_ragged': (c_int, [POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int)]),
    'tts_device_info': (c_int, [c_void_p, c_char_p, POINTER(c_int)]),
}

_lib = None


def exported_symbols():
    """Names every include/sstts_hip.h entry point must resolve to."""
    return sorted(_PROTOTYPES)


def load_library(path=None):
    """dlopen the HIP library (no GPU needed for this) and attach prototypes."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise OSError('{} not found: build it with `python single-speaker-tts_amd/build.py` '
                      '(there is no CPU fallback)'.format(path))
    lib = ctypes.CDLL(path)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class DeviceArray(object):
    """A typed device buffer owned by the library allocator."""

    def __init__(self, engine, shape, dtype=np.float32):
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = c_void_p()
        # allocated on the engine's device, whatever device is current on this thread
        rc = engine.lib.tts_device_malloc(engine.handle, byref(p), self.nbytes)
        if rc != TTS_OK:
            raise TtsError(rc, 'tts_device_malloc({}) failed'.format(self.nbytes))
        self.ptr = p.value

    def data_ptr(self):
        return self.ptr

    def copy_from(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes, (host.shape, self.shape)
        self.engine._check(self.engine.lib.tts_memcpy_h2d(self.engine.handle, self.ptr, host.ctypes.data,
                                                          self.nbytes))
        return self

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        self.engine._check(self.engine.lib.tts_memcpy_d2h(self.engine.handle, out.ctypes.data, self.ptr,
                                                          self.nbytes))
        return out

    def free(self):
        if self.ptr:
            if getattr(self.engine, 'handle', None):
                self.engine.lib.tts_device_free(self.engine.handle, self.ptr)
            else:   # the engine is gone (tts_destroy does not free caller-owned buffers)
                self.engine.lib.tts_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _is_device(x):
    return hasattr(x, 'data_ptr') and not isinstance(x, np.ndarray)


def _int32_ptr(a):
    """a host int32 array as the ``const int32_t*`` of a call; None: NULL"""
    return a.ctypes.data_as(POINTER(c_int32)) if a is not None else None


def _checked_lengths(lengths, hi, name, bound, lo=1):
    """Host lengths -- an integer array of the batch's shape already -- as a contiguous int32 array, every one in ``lo`` .. ``hi``
    (``lo`` 0: a row may hold nothing); the ValueError speaks of the caller's argument ``name`` and of its ``bound``."""
    for b, n in enumerate(lengths.tolist()):
        if not lo <= n <= hi:
            raise ValueError('{}[{}] = {} is not in {} .. {} = {}'.format(name, b, n, lo, bound, hi))
    return np.ascontiguousarray(lengths, dtype=np.int32)


def _sample_lengths(n_samples, B, n, lo=1):
    """``n_samples`` of a call on B rows of n samples -- None, or B host integers in ``lo`` .. n -- as None or a checked int32 array"""
    if n_samples is None:
        return None
    ns = np.asarray(n_samples)
    if ns.shape != (B,) or ns.dtype.kind not in 'iu':
        raise ValueError('n_samples: {} integers are needed, got shape {} of {}'.format(B, ns.shape, ns.dtype))
    return _checked_lengths(ns, n, 'n_samples', 'n', lo)


def _records(buf, record):
    """a device buffer of B records -- (B, k) of a plain type -- as the host array (B,) of ``record``; the buffer is freed"""
    host = buf.to_host().view(record).reshape(-1)
    buf.free()
    return host


def _waveforms(what, wavs, uniform=False):
    """``wavs`` -- one waveform (n,) or a batch (B, n), host or device -- as ``(wavs, single, B, n)``: a 1-D host array becomes
    one row, a 1-D device buffer is one row as it lies.  ``uniform``: the compositions' rule -- two dimensions from here on (no
    1-D device buffer), and whether the signal is long enough is theirs to say."""
    single = len(wavs.shape) == 1
    if single and not _is_device(wavs):
        wavs = np.asarray(wavs).reshape(1, -1)
    if (len(wavs.shape) != 2) if uniform else (len(wavs.shape) not in (1, 2) or min(wavs.shape) < 1):
        raise ValueError('{}: one waveform (n,) or a {}batch (B, n) is needed, got shape {}'.format(
            what, 'uniform ' if uniform else '', tuple(wavs.shape)))
    B, n = (1, int(wavs.shape[0])) if len(wavs.shape) == 1 else (int(d) for d in wavs.shape)
    return wavs, single, B, n


def ragged_frame_counts(n_frames, B, T_max, hop_length, n_fft):
    """The ``n_frames`` argument of a ragged Griffin-Lim call as a contiguous int32 array of B lengths, checked as
    tts_griffin_lim_ragged checks them (ValueError, raised before a handle is touched): 1 <= n_frames[b] <= T_max and a
    signal longer than the reflect padding, hop (n_frames[b] - 1) > n_fft / 2."""
    nf = np.ascontiguousarray(np.asarray(n_frames).reshape(-1), dtype=np.int32)
    if nf.shape[0] != B:
        raise ValueError('n_frames: {} lengths for a batch of {}'.format(nf.shape[0], B))
    for b, n in enumerate(nf.tolist()):
        if not 1 <= n <= T_max:
            raise ValueError('n_frames[{}] = {} is not in 1 .. T_max = {}'.format(b, n, T_max))
        if hop_length * (n - 1) <= n_fft // 2:
            raise ValueError('n_frames[{}] = {}: the signal is shorter than n_fft / 2 (reflect padding undefined)'.format(b, n))
    return nf


def momentum_thousandths(momentum):
    """The ``gl_momentum`` option value of a fast Griffin-Lim momentum in [0, 1): thousandths, 0 .. 999.  Anything else
    (a NaN included) is a ValueError -- raised here, before a handle is touched."""
    m = float(momentum)
    if not 0.0 <= m < 1.0:
        raise ValueError('momentum must be in [0, 1), got {!r}'.format(momentum))
    return min(999, int(round(m * 1000.0)))


PHASE_INIT_VALUES = {'random': 0, 'estimate': 1}


def phase_init_value(phase_init):
    """``phase_init`` of the Griffin-Lim and synthesis calls as the ``gl_init`` option value: 'random' -> 0 (phases drawn
    from the seed, or the caller's ``init_phase``), 'estimate' -> 1 (phases estimated from the call's own magnitudes,
    tts_phase_estimate); None stays None (the handle's option as it stands).  Anything else is a ValueError -- raised here,
    before a handle is touched."""
    if phase_init is None:
        return None
    if not isinstance(phase_init, str) or phase_init not in PHASE_INIT_VALUES:
        raise ValueError("phase_init must be None, 'random' or 'estimate', got {!r}".format(phase_init))
    return PHASE_INIT_VALUES[phase_init]


def phase_init_kwargs(engine, phase_init):
    """The keyword a wrapper that states the start of every call hands to ``engine.griffin_lim``: none where the engine's
    ``gl_init`` option already is what the call asks for (any engine-like object serves the default), ``phase_init=...`` where
    the call has to switch it."""
    v = phase_init_value(phase_init)
    if v is None or v == getattr(engine, '_gl_init', 0):
        return {}
    return {'phase_init': phase_init}


def phase_estimate_args(shape, n_fft, hop_length, n_frames, time_major=False):
    """The checked arguments of a phase-estimate call on an array of ``shape`` -- (B, F, T), or (B, T, F) time-major:
    ``(B, T, F, n_frames)`` with n_frames a contiguous int32 array or None.  ValueError, raised before a handle is touched,
    for what tts_phase_estimate refuses."""
    if int(n_fft) != n_fft or not 256 <= n_fft <= 4096 or (int(n_fft) & (int(n_fft) - 1)):
        raise ValueError('phase_estimate: n_fft must be a power of two between 256 and 4096, got {!r}'.format(n_fft))
    if int(hop_length) != hop_length or not 1 <= hop_length <= n_fft:
        raise ValueError('phase_estimate: need 1 <= hop_length <= n_fft, got {!r}'.format(hop_length))
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('phase_estimate: a non-empty 3-D array is needed, got shape {}'.format(tuple(shape)))
    B = int(shape[0])
    T, F = (int(shape[1]), int(shape[2])) if time_major else (int(shape[2]), int(shape[1]))
    if F != 1 + int(n_fft) // 2:
        raise ValueError('phase_estimate: {} bins given, n_fft = {} has {}'.format(F, n_fft, 1 + int(n_fft) // 2))
    return B, T, F, stretch_frame_counts(n_frames, B, T)


def stop_at_silence_setting(stop_at_silence):
    """``stop_at_silence`` of the synthesis calls -- None (off) or ``(threshold_db, keep_frames)`` -- as a checked tuple
    ``(float, int)`` or None.  ValueError, raised before a handle is touched, for anything else: a NaN threshold, a negative
    or non-integral keep_frames (tts_set_end_of_speech refuses the same)."""
    if stop_at_silence is None:
        return None
    try:
        threshold_db, keep_frames = stop_at_silence
    except (TypeError, ValueError):
        raise ValueError('stop_at_silence must be None or (threshold_db, keep_frames), got {!r}'.format(stop_at_silence))
    threshold_db = float(threshold_db)
    if threshold_db != threshold_db:
        raise ValueError('stop_at_silence: threshold_db is NaN')
    if int(keep_frames) != keep_frames or keep_frames < 0:
        raise ValueError('stop_at_silence: keep_frames must be an integer >= 0, got {!r}'.format(keep_frames))
    return threshold_db, int(keep_frames)


def silence_keep_frames(keep_samples, hop_length):
    """Whole frames that cover ``keep_samples`` samples of audio (the caller's ms_to_samples of its milliseconds): rounded up."""
    if not keep_samples >= 0 or hop_length < 1:
        raise ValueError('the audio kept behind the speech must be >= 0 samples, got {!r} (hop {!r})'.format(keep_samples, hop_length))
    return -(-int(keep_samples) // int(hop_length))


SPEAKING_RATE_MIN, SPEAKING_RATE_MAX = 0.25, 4.0


def speaking_rate_value(rate):
    """``speaking_rate`` of the synthesis and stretch calls as a checked float (None stays None: the handle's setting as it
    stands).  ValueError, raised before a handle is touched, for what tts_set_speaking_rate refuses: a rate that is not
    finite or lies outside [0.25, 4]."""
    if rate is None:
        return None
    try:
        r = float(rate)
    except (TypeError, ValueError):
        raise ValueError('speaking_rate must be a number in [0.25, 4], got {!r}'.format(rate))
    if not SPEAKING_RATE_MIN <= r <= SPEAKING_RATE_MAX:   # (a NaN fails both comparisons)
        raise ValueError('speaking_rate must be finite and lie in [0.25, 4], got {!r}'.format(rate))
    return r


def stretched_frames(n, rate):
    """tts_stretched_frames on the host: ceil(n / rate) in double = len(np.arange(0, n, rate, dtype=float)), the frames a
    time-stretched utterance of ``n`` frames has (reference audio/effects.py:46-88, librosa 0.6 phase_vocoder)."""
    r = speaking_rate_value(rate)
    if r is None or int(n) != n or n < 1:
        raise ValueError('stretched_frames: need n >= 1 frames and a rate, got {!r}, {!r}'.format(n, rate))
    return int(np.ceil(np.float64(int(n)) / np.float64(r)))


F0_MAX_WINDOW = 2048   # tts_f0_max_window()
F0_MAX_LAG = 1024      # tts_f0_max_lag()


def f0_lag_bounds(sampling_rate, fmin, fmax):
    """(tau_min, tau_max) of an F0 search between ``fmin`` and ``fmax`` Hz: max(2, int(sr // fmax)) and ceil(sr / fmin)."""
    sr, fmin, fmax = float(sampling_rate), float(fmin), float(fmax)
    if not (np.isfinite(sr) and sr > 0 and np.isfinite(fmin) and np.isfinite(fmax) and 0 < fmin <= fmax):
        raise ValueError('f0: need a positive finite sampling rate and 0 < fmin <= fmax, got {!r}, {!r}, {!r}'.format(sampling_rate, fmin, fmax))
    return max(2, int(sr // fmax)), int(np.ceil(sr / fmin))


def f0_frames(n, hop_length):
    """tts_f0_frames: the values tts_f0 writes for ``n`` samples, 1 + n // hop_length."""
    return 1 + int(n) // int(hop_length)


STOI_RATE = 10000          # the analysis rate of tts_stoi
STOI_BANDS = 15
STOI_MAX_FRAMES = 65536    # tts_stoi_max_frames()
STOI_RECORD = np.dtype([('frames', np.int32), ('kept', np.int32), ('segments', np.int32), ('degenerate', np.int32), ('value', np.float64)])


def stoi_frames(n):
    """tts_stoi_frames: the frames of 256 samples, 128 apart, in ``n`` samples -- 0 below 256."""
    n = int(n)
    return 0 if n < 256 else (n - 256) // 128 + 1


LOUDNESS_SR_MIN, LOUDNESS_SR_MAX = 8000, 192000   # what tts_loudness takes
LOUDNESS_TARGET, LOUDNESS_MAX_PEAK = -23.0, 1.0   # EBU R 128's programme level, and full scale


def loudness_sampling_rate(what, sampling_rate):
    """the sampling rate of a loudness call as a checked int; ValueError, raised before a handle is touched, for what the
    library refuses: a rate that is not an integer in 8000 .. 192000"""
    try:
        ok = int(sampling_rate) == sampling_rate and LOUDNESS_SR_MIN <= sampling_rate <= LOUDNESS_SR_MAX
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('{}: the sampling rate must be an integer in {} .. {}, got {!r}'.format(what, LOUDNESS_SR_MIN, LOUDNESS_SR_MAX, sampling_rate))
    return int(sampling_rate)


def loudness_target(what, target_lufs, max_peak):
    """(target_lufs, max_peak) as checked floats; ValueError for a target that is not finite or a ceiling that is not finite and
    positive (tts_loudness_normalize refuses the same)"""
    try:
        t, p = float(target_lufs), float(max_peak)
    except (TypeError, ValueError):
        raise ValueError('{}: target_lufs and max_peak must be numbers, got {!r}, {!r}'.format(what, target_lufs, max_peak))
    if not np.isfinite(t):
        raise ValueError('{}: the target must be a finite number of LUFS, got {!r}'.format(what, target_lufs))
    if not (np.isfinite(p) and p > 0):
        raise ValueError('{}: max_peak must be finite and positive, got {!r}'.format(what, max_peak))
    return t, p


def loudness_setting(loudness):
    """``loudness`` of the synthesis calls -- None (the handle's setting as it stands), a target in LUFS or ``(target_lufs,
    max_peak)`` -- as None or a checked tuple ``(target_lufs, max_peak)``.  ValueError, raised before a handle is touched, for
    anything else."""
    if loudness is None:
        return None
    if isinstance(loudness, (tuple, list)):
        if len(loudness) != 2:
            raise ValueError('loudness must be None, a target in LUFS or (target_lufs, max_peak), got {!r}'.format(loudness))
        return loudness_target('loudness', loudness[0], loudness[1])
    return loudness_target('loudness', loudness, LOUDNESS_MAX_PEAK)


def lufs(mean_square):
    """-0.691 + 10 log10(z) of the mean squares tts_loudness returns: -inf for 0 (nothing passed the gates), NaN for NaN"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return -0.691 + 10.0 * np.log10(np.asarray(mean_square, dtype=np.float64))


def loudness_filter(sampling_rate):
    """tts_loudness_filter: b0 b1 b2 a1 a2 of the K-weighting shelf, then of its high-pass, as the library designed them for
    ``sampling_rate`` (float64 (10,)); needs no device"""
    sr = loudness_sampling_rate('loudness_filter', sampling_rate)
    out = (ctypes.c_double * 10)()
    rc = load_library().tts_loudness_filter(sr, out)
    if rc != TTS_OK:
        raise TtsError(rc, 'tts_loudness_filter({}) refused'.format(sr))
    return np.array(out[:], dtype=np.float64)


LIMIT_MAX_LOOKAHEAD = 1024       # tts_limit_max_lookahead(), samples
LIMIT_LOOKAHEAD_MS = 5.0         # the look-ahead of a limiter given as a bare ceiling
LIMIT_OVERSAMPLE = 4             # ... and its mode: the interpolated peaks


def limit_arguments(what, ceiling, lookahead, oversample):
    """(ceiling, lookahead, oversample) of a tts_limit call as a checked float and two ints; ValueError, raised before a handle is
    touched, for what the library refuses: a ceiling that is not finite and positive, a look-ahead that is not an integer in
    0 .. 1024 samples, an oversample other than 1 or 4"""
    try:
        c = float(ceiling)
    except (TypeError, ValueError):
        raise ValueError('{}: the ceiling must be a number, got {!r}'.format(what, ceiling))
    if not (np.isfinite(c) and c > 0):
        raise ValueError('{}: the ceiling must be finite and positive, got {!r}'.format(what, ceiling))
    try:
        ok = int(lookahead) == lookahead and 0 <= lookahead <= LIMIT_MAX_LOOKAHEAD
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('{}: the look-ahead must be an integer in 0 .. {} samples, got {!r}'.format(what, LIMIT_MAX_LOOKAHEAD, lookahead))
    if isinstance(oversample, (bool, np.bool_)) or oversample not in (1, 4):
        raise ValueError('{}: oversample must be 1 or 4, got {!r}'.format(what, oversample))
    return c, int(lookahead), int(oversample)


def limiter_setting(limiter):
    """``limiter`` of the synthesis calls -- None (the handle's setting as it stands), a ceiling or ``(ceiling, lookahead_ms,
    oversample)`` -- as None or a checked tuple ``(ceiling, lookahead_ms, oversample)``; a bare ceiling looks 5 ms ahead at the
    interpolated peaks.  ValueError, raised before a handle is touched, for anything else.  (The look-ahead becomes samples at the
    engine's sampling rate, where more than 1024 of them are refused: ``limiter_lookahead``.)"""
    if limiter is None:
        return None
    if isinstance(limiter, (tuple, list)):
        if len(limiter) != 3:
            raise ValueError('limiter must be None, a ceiling or (ceiling, lookahead_ms, oversample), got {!r}'.format(limiter))
        ceiling, ms, oversample = limiter
    else:
        ceiling, ms, oversample = limiter, LIMIT_LOOKAHEAD_MS, LIMIT_OVERSAMPLE
    if isinstance(ceiling, (bool, np.bool_)):
        raise ValueError('limiter: the ceiling must be a number, got {!r}'.format(ceiling))
    c, _l, o = limit_arguments('limiter', ceiling, 0, oversample)
    try:
        ms = float(ms)
    except (TypeError, ValueError):
        raise ValueError('limiter: the look-ahead must be a number of milliseconds, got {!r}'.format(limiter[1]))
    if not (np.isfinite(ms) and ms >= 0):
        raise ValueError('limiter: the look-ahead must be finite and not negative, got {!r}'.format(ms))
    return c, ms, o


def limiter_lookahead(what, lookahead_ms, sampling_rate):
    """a look-ahead in milliseconds as samples at ``sampling_rate``, rounded to the nearest; ValueError above 1024 samples"""
    L = int(round(float(lookahead_ms) * 1e-3 * float(sampling_rate)))
    if not 0 <= L <= LIMIT_MAX_LOOKAHEAD:
        raise ValueError('{}: a look-ahead of {} ms is {} samples at {} Hz, more than {}'.format(what, lookahead_ms, L, sampling_rate, LIMIT_MAX_LOOKAHEAD))
    return L


def dbtp(peak):
    """20 log10 of the peaks tts_true_peak returns: -inf for 0"""
    with np.errstate(divide='ignore'):
        return 20.0 * np.log10(np.asarray(peak, dtype=np.float64))


def true_peak_filter():
    """tts_true_peak_filter: the taps h[phase][tap] of the 4x interpolation as the library designed them (float64 (4, 12)); needs
    no device"""
    out = (ctypes.c_double * 48)()
    rc = load_library().tts_true_peak_filter(out)
    if rc != TTS_OK:
        raise TtsError(rc, 'tts_true_peak_filter refused')
    return np.array(out[:], dtype=np.float64).reshape(4, 12)


# ---- the equaliser (csrc/equalizer_plan.h): the kinds of a section, the limits of a design and the profiles.  Every preset is
# untuned: nobody has listened to one.
EQ_MAX_SECTIONS = 8              # tts_equalizer_max_sections()
EQ_KINDS = {'lowpass': 0, 'highpass': 1, 'peak': 2, 'lowshelf': 3, 'highshelf': 4}
EQ_KIND_NAMES = {v: k for k, v in EQ_KINDS.items()}
EQ_SR_MIN, EQ_SR_MAX = 8000, 192000
EQ_F_MIN, EQ_F_MAX = 1e-4, 0.49      # f0 / sr
EQ_Q_MIN, EQ_Q_MAX = 0.1, 30.0
EQ_GAIN_MIN, EQ_GAIN_MAX = -40.0, 24.0
EQ_Q_BUTTER2 = 0.7071067811865476    # one low- or high-pass section: 2nd-order Butterworth; the default Q
EQ_Q_BUTTER4 = (0.5411961001461969, 1.3065629648763766)   # two of them: 4th-order Butterworth
EQ_PROFILES = collections.OrderedDict((
    ('telephony', (('highpass', 300.0, EQ_Q_BUTTER4[0], 0.0), ('highpass', 300.0, EQ_Q_BUTTER4[1], 0.0),
                   ('lowpass', 3400.0, EQ_Q_BUTTER4[0], 0.0), ('lowpass', 3400.0, EQ_Q_BUTTER4[1], 0.0))),
    ('small-speaker', (('highpass', 150.0, EQ_Q_BUTTER4[0], 0.0), ('highpass', 150.0, EQ_Q_BUTTER4[1], 0.0), ('peak', 3000.0, 1.0, 3.0))),
    ('rumble', (('highpass', 20.0, 0.7071, 0.0),)),
    ('bright', (('highshelf', 6000.0, EQ_Q_BUTTER2, 3.0),)),
    ('warm', (('highshelf', 6000.0, EQ_Q_BUTTER2, -3.0), ('lowshelf', 200.0, EQ_Q_BUTTER2, 2.0))),
))


def equalizer_design(kind, sampling_rate, f0_hz, q=EQ_Q_BUTTER2, gain_db=0.0):
    """One section ``(b0, b1, b2, a1, a2)``, normalised by a0, as tts_equalizer_design makes it (csrc/equalizer_plan.h: the
    bilinear transform in its tan form), in Python floats; needs no library.  ``kind``: a name of ``EQ_KINDS`` or its number.
    ValueError: a kind, sampling rate, f0 / sr, Q or gain outside the limits."""
    k = EQ_KINDS.get(kind, kind) if isinstance(kind, str) else kind
    if isinstance(k, bool) or k not in EQ_KIND_NAMES:
        raise ValueError('equalizer: the kind must be one of {}, got {!r}'.format(', '.join(EQ_KINDS), kind))
    sr = sampling_rate
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or not EQ_SR_MIN <= sr <= EQ_SR_MAX:
        raise ValueError('equalizer: the sampling rate must be an integer in {} .. {}, got {!r}'.format(EQ_SR_MIN, EQ_SR_MAX, sr))
    try:
        f0, q, g = float(f0_hz), float(EQ_Q_BUTTER2 if q is None else q), float(0.0 if gain_db is None else gain_db)
    except (TypeError, ValueError):
        raise ValueError('equalizer: f0, Q and the gain must be numbers, got {!r}'.format((f0_hz, q, gain_db)))
    if not EQ_F_MIN * sr <= f0 <= EQ_F_MAX * sr:   # (against the products: f0 = 0.49 * sr is inside)
        raise ValueError('equalizer: {} at {:g} Hz: f0 / sr = {:g} at {} Hz is not in {:g} .. {:g}'.format(EQ_KIND_NAMES[k], f0, f0 / sr, sr, EQ_F_MIN, EQ_F_MAX))
    if not EQ_Q_MIN <= q <= EQ_Q_MAX:
        raise ValueError('equalizer: Q = {:g} is not in {:g} .. {:g}'.format(q, EQ_Q_MIN, EQ_Q_MAX))
    if k >= 2 and not EQ_GAIN_MIN <= g <= EQ_GAIN_MAX:
        raise ValueError('equalizer: a gain of {:g} dB is not in {:g} .. {:g}'.format(g, EQ_GAIN_MIN, EQ_GAIN_MAX))
    K = math.tan(math.pi * f0 / sr)
    KK, KQ = K * K, K / q
    if k < 2:
        a0, a1, a2 = 1.0 + KQ + KK, 2.0 * (KK - 1.0), 1.0 - KQ + KK
        b0, b1 = (KK, 2.0 * KK) if k == 0 else (1.0, -2.0)
        b2 = b0
    elif k == 2:
        A = 10.0 ** (g / 40.0)
        b0, b1, b2 = 1.0 + KQ * A + KK, 2.0 * (KK - 1.0), 1.0 - KQ * A + KK
        a0, a1, a2 = 1.0 + KQ / A + KK, b1, 1.0 - KQ / A + KK
    else:
        A = 10.0 ** (g / 40.0)
        s = math.sqrt(A) * KQ
        lift, rest, lift_m, rest_m = 1.0 + A * KK, A + KK, 2.0 * (A * KK - 1.0), 2.0 * (KK - A)
        if k == 3:
            b0, b1, b2, a0, a1, a2 = A * (lift + s), A * lift_m, A * (lift - s), rest + s, rest_m, rest - s
        else:
            b0, b1, b2, a0, a1, a2 = A * (rest + s), A * rest_m, A * (rest - s), lift + s, lift_m, lift - s
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def equalizer_profile(name, sampling_rate):
    """The sections of a profile of ``EQ_PROFILES`` at a sampling rate, float64 (S, 5), as tts_equalizer_profile makes them.
    ValueError: an unknown name, or a corner that does not fit under 0.49 sr (the message names the profile)."""
    if name not in EQ_PROFILES:
        raise ValueError('equalizer: no profile {!r} (there are: {})'.format(name, ', '.join(EQ_PROFILES)))
    try:
        return np.array([equalizer_design(k, sampling_rate, f0, q, g) for k, f0, q, g in EQ_PROFILES[name]], dtype=np.float64)
    except ValueError as e:
        raise ValueError("equalizer: the profile '{}' does not fit {} Hz: {}".format(name, sampling_rate, e))


def equalizer_sos_check(what, sos):
    """``sos`` as float64 (S, 5) rows b0 b1 b2 a1 a2, checked as tts_equalize checks them; ValueError before a handle is touched"""
    try:
        a = np.array(sos, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('{}: sections of five numbers b0 b1 b2 a1 a2 are needed, got {!r}'.format(what, sos))
    if a.ndim != 2 or a.shape[1] != 5 or not 1 <= a.shape[0] <= EQ_MAX_SECTIONS:
        raise ValueError('{}: 1 .. {} sections of five numbers b0 b1 b2 a1 a2 are needed, got shape {}'.format(what, EQ_MAX_SECTIONS, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError('{}: every coefficient must be finite'.format(what))
    for i, (a1, a2) in enumerate(a[:, 3:]):
        if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
            raise ValueError('{}: section {} is not stable: |a2| < 1 and |a1| < 1 + a2 are needed'.format(what, i))
    return np.ascontiguousarray(a)


def equalizer_setting(equalizer):
    """``equalizer`` of the synthesis calls -- None (the handle's setting as it stands), a profile name of ``EQ_PROFILES``, a list
    of ``(kind, f0_hz[, q[, gain_db]])`` sections (Q 0.7071..., 0 dB where left out) or an (S, 5) array of sections b0 b1 b2 a1
    a2 -- as what the mirror holds: None, ``('profile', name)``, ``('design', ((kind, f0, q, gain_db), ...))`` or ``('sos', ((b0,
    b1, b2, a1, a2), ...))``.  ValueError before a handle is touched; what depends on the sampling rate is checked where the rate
    is known (``equalizer_sections``)."""
    if equalizer is None:
        return None
    if isinstance(equalizer, str):
        if equalizer not in EQ_PROFILES:
            raise ValueError('equalizer: no profile {!r} (there are: {})'.format(equalizer, ', '.join(EQ_PROFILES)))
        return ('profile', equalizer)
    if isinstance(equalizer, tuple) and len(equalizer) == 2 and equalizer[0] in ('profile', 'design', 'sos') and not isinstance(equalizer[1], (int, float)):
        return equalizer_setting(equalizer[1])   # (a checked value: checked again)
    if isinstance(equalizer, np.ndarray) or (isinstance(equalizer, (list, tuple)) and len(equalizer) and
                                             all(isinstance(r, (list, tuple, np.ndarray)) and len(r) == 5 and not isinstance(r[0], str) for r in equalizer)):
        return ('sos', tuple(tuple(float(v) for v in row) for row in equalizer_sos_check('equalizer', equalizer)))
    if not isinstance(equalizer, (list, tuple)) or not 1 <= len(equalizer) <= EQ_MAX_SECTIONS:
        raise ValueError('equalizer must be None, a profile name, 1 .. {} (kind, f0_hz, q, gain_db) sections or an (S, 5) array, got {!r}'.format(
            EQ_MAX_SECTIONS, equalizer))
    rows = []
    for row in equalizer:
        if not isinstance(row, (list, tuple)) or not 2 <= len(row) <= 4:
            raise ValueError('equalizer: a section is (kind, f0_hz[, q[, gain_db]]), got {!r}'.format(row))
        kind, f0 = row[0], row[1]
        q = row[2] if len(row) > 2 and row[2] is not None else EQ_Q_BUTTER2
        g = row[3] if len(row) > 3 and row[3] is not None else 0.0
        k = EQ_KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(k, bool) or k not in EQ_KIND_NAMES:
            raise ValueError('equalizer: the kind must be one of {}, got {!r}'.format(', '.join(EQ_KINDS), kind))
        equalizer_design(k, 48000, 1000.0, q, g)   # (Q and the gain; f0 waits for the rate)
        if isinstance(f0, bool) or not isinstance(f0, (int, float, np.integer, np.floating)) or not (math.isfinite(f0) and f0 > 0):
            raise ValueError('equalizer: f0 must be a positive number of Hz, got {!r}'.format(f0))
        rows.append((EQ_KIND_NAMES[k], float(f0), float(q), float(g)))
    return ('design', tuple(rows))


def equalizer_sections(setting, sampling_rate):
    """the sections, float64 (S, 5), of a checked ``equalizer_setting`` at a sampling rate; ValueError where a corner does not fit"""
    how, what = setting
    if how == 'profile':
        return equalizer_profile(what, sampling_rate)
    if how == 'design':
        return np.array([equalizer_design(k, sampling_rate, f0, q, g) for k, f0, q, g in what], dtype=np.float64)
    return equalizer_sos_check('equalizer', what)


# ---- the compressor (csrc/compressor_plan.h): the limits of its parameters and the profiles.  Every preset is untuned: nobody has
# listened to one.
CMP_THRESHOLD_MIN, CMP_THRESHOLD_MAX = -80.0, 0.0      # dB re full scale
CMP_KNEE_MAX = 40.0
CMP_MAKEUP_MIN, CMP_MAKEUP_MAX = -24.0, 24.0
CMP_MS_MAX = 10000.0
# threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db
CMP_PROFILES = collections.OrderedDict((
    ('speech', (-18.0, 3.0, 6.0, 5.0, 100.0, 3.0)),
    ('telephony', (-20.0, 4.0, 6.0, 3.0, 80.0, 6.0)),
    ('small-speaker', (-24.0, 6.0, 10.0, 2.0, 60.0, 8.0)),
))
CMP_DEFAULTS = (None, None, 6.0, 5.0, 100.0, 0.0)     # what a short tuple leaves out: knee, attack, release, make-up
COMPRESS_RECORD = np.dtype([('n', np.int32), ('reduced', np.int32), ('max_reduction_db', np.float32), ('peak_out', np.float32)])


class TtsCompressor(ctypes.Structure):
    """tts_compressor_t"""
    _fields_ = [(name, ctypes.c_double) for name in ('threshold_db', 'slope', 'knee_db', 'makeup_db', 'attack_coeff', 'release_coeff')]


def compressor_design(sampling_rate, attack_ms, release_ms):
    """``(attack_coeff, release_coeff)`` as tts_compressor_design makes them, exp(-1 / (ms * 1e-3 * sr)) and 0 for 0 ms, in Python
    floats; needs no library.  ValueError: a sampling rate or a time outside the limits."""
    sr = sampling_rate
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or not EQ_SR_MIN <= sr <= EQ_SR_MAX:
        raise ValueError('compressor: the sampling rate must be an integer in {} .. {}, got {!r}'.format(EQ_SR_MIN, EQ_SR_MAX, sr))
    out = []
    for what, ms in (('attack', attack_ms), ('release', release_ms)):
        if not 0.0 <= ms <= CMP_MS_MAX:
            raise ValueError('compressor: the {} of {!r} ms is not in 0 .. {:g}'.format(what, ms, CMP_MS_MAX))
        out.append(0.0 if ms == 0 else math.exp(-1.0 / (ms * 1e-3 * sr)))
    return tuple(out)


def compressor_params_check(what, values):
    """``(threshold_db, slope, knee_db, makeup_db, attack_coeff, release_coeff)`` as six floats, checked as tts_compress checks them"""
    try:
        T, slope, W, makeup, aA, aR = (float(v) for v in values)
    except (TypeError, ValueError):
        raise ValueError('{}: threshold_db, slope, knee_db, makeup_db, attack_coeff and release_coeff are needed, got {!r}'.format(what, values))
    for name, v, lo, hi in (('threshold_db', T, CMP_THRESHOLD_MIN, CMP_THRESHOLD_MAX), ('slope', slope, 0.0, 1.0), ('knee_db', W, 0.0, CMP_KNEE_MAX),
                            ('makeup_db', makeup, CMP_MAKEUP_MIN, CMP_MAKEUP_MAX)):
        if not lo <= v <= hi:
            raise ValueError('{}: {} = {!r} is not in {:g} .. {:g}'.format(what, name, v, lo, hi))
    for name, v in (('attack_coeff', aA), ('release_coeff', aR)):
        if not 0.0 <= v < 1.0:
            raise ValueError('{}: {} = {!r} is not in [0, 1)'.format(what, name, v))
    return (T, slope, W, makeup, aA, aR)


def compressor_setting(compressor):
    """``compressor`` of the synthesis calls -- None (the handle's setting as it stands), a profile name of ``CMP_PROFILES``, or
    ``(threshold_db, ratio[, knee_db[, attack_ms[, release_ms[, makeup_db]]]])`` (ratio >= 1, inf allowed; 6 dB, 5 ms, 100 ms and
    0 dB where left out) -- as what the mirror holds: None, ``('profile', name)``, ``('design', (T, ratio, knee, attack_ms,
    release_ms, makeup))`` or, for coefficients made elsewhere, ``('params', (threshold_db, slope, knee_db, makeup_db, attack_coeff,
    release_coeff))``.  ValueError before a handle is touched; the coefficients are made where the rate is known
    (``compressor_params``)."""
    if compressor is None:
        return None
    if isinstance(compressor, str):
        if compressor not in CMP_PROFILES:
            raise ValueError('compressor: no profile {!r} (there are: {})'.format(compressor, ', '.join(CMP_PROFILES)))
        return ('profile', compressor)
    if isinstance(compressor, tuple) and len(compressor) == 2 and compressor[0] in ('profile', 'design', 'params'):
        if compressor[0] == 'params':
            return ('params', compressor_params_check('compressor', compressor[1]))
        return compressor_setting(compressor[1])   # (a checked value: checked again)
    if not isinstance(compressor, (list, tuple)) or not 2 <= len(compressor) <= 6:
        raise ValueError('compressor must be None, a profile name or (threshold_db, ratio[, knee_db[, attack_ms[, release_ms[, makeup_db]]]]), '
                         'got {!r}'.format(compressor))
    values = [CMP_DEFAULTS[i] if i >= len(compressor) or compressor[i] is None else compressor[i] for i in range(6)]
    if any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) for v in values):
        raise ValueError('compressor: threshold, ratio, knee, attack, release and make-up must be numbers, got {!r}'.format(compressor))
    T, ratio, W, attack, release, makeup = (float(v) for v in values)
    if not ratio >= 1.0:
        raise ValueError('compressor: the ratio must be 1 or more (inf: a hard ceiling on the envelope), got {!r}'.format(ratio))
    compressor_params_check('compressor', (T, 1.0 / ratio, W, makeup, 0.0, 0.0))
    compressor_design(48000, attack, release)
    return ('design', (T, ratio, W, attack, release, makeup))


def compressor_params(setting, sampling_rate):
    """the six parameters of a checked ``compressor_setting`` at a sampling rate"""
    how, what = setting
    if how == 'params':
        return compressor_params_check('compressor', what)
    T, ratio, W, attack, release, makeup = CMP_PROFILES[what] if how == 'profile' else what
    aA, aR = compressor_design(sampling_rate, attack, release)
    return compressor_params_check('compressor', (T, 1.0 / ratio, W, makeup, aA, aR))


# ---- the watermark (csrc/watermark_plan.h): the limits of its parameters.  The defaults are UNTUNED: no trained checkpoint was at
# hand and nobody has listened -- they say neither that the mark is inaudible nor that it survives a given channel.
WM_BITS_MAX = 32
WM_CHIP_MIN, WM_CHIP_MAX = 2, 16
WM_SYMBOL_MAX = 65536
WM_STRENGTH_MAX = 0.25
WM_MAX_OFFSETS = 4096
WM_DEFAULTS = (None, 0, 16, 8, 64, 0.02)     # what a short tuple leaves out: payload, payload_bits, chip, chips_per_symbol, strength
# The detection threshold on zeta, measured on the CPU oracle (tests/test_watermark_host.py): 1.5 times the largest
# zeta of 200 wrong keys on every signal of tests/watermark_cases.py at D = 64
WM_THRESHOLD = 6.6
WATERMARK_EMBED_RECORD = np.dtype([('n', np.int32), ('marked', np.int32), ('peak_out', np.float32), ('spare', np.int32)])
WATERMARK_DETECT_RECORD = np.dtype([('offset', np.int32), ('n', np.int32), ('score', np.int64), ('energy', np.int64), ('payload', np.uint32),
                                    ('spare', np.uint32)])


class TtsWatermark(ctypes.Structure):
    """tts_watermark_t"""
    _fields_ = [('key', ctypes.c_uint64), ('payload', ctypes.c_uint32), ('payload_bits', c_int32), ('chip', c_int32),
                ('chips_per_symbol', c_int32), ('strength', ctypes.c_double)]


def watermark_setting(watermark):
    """``watermark`` of the synthesis calls and of ``watermark_embed`` / ``watermark_detect`` -- None (the handle's setting as it
    stands), a key (an integer in 0 .. 2^64 - 1), ``(key, payload)`` or ``(key, payload, payload_bits, chip, chips_per_symbol,
    strength)`` (16 bits, 8 samples a chip, 64 chips a symbol and 0.02 where left out: UNTUNED defaults) -- as what the mirror
    holds: None or the six values, checked as tts_watermark_embed checks them.  ValueError before a handle is touched."""
    if watermark is None:
        return None
    values = (watermark,) if isinstance(watermark, (int, np.integer)) and not isinstance(watermark, (bool, np.bool_)) else watermark
    if not isinstance(values, (list, tuple)) or not 1 <= len(values) <= 6:
        raise ValueError('watermark must be None, a key, (key, payload) or (key, payload, payload_bits, chip, chips_per_symbol, strength), '
                         'got {!r}'.format(watermark))
    values = [WM_DEFAULTS[i] if i >= len(values) or values[i] is None else values[i] for i in range(6)]
    for name, v in zip(('key', 'payload', 'payload_bits', 'chip', 'chips_per_symbol'), values):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError('watermark: {} must be an integer, got {!r}'.format(name, v))
    key, payload, P, L, C = (int(v) for v in values[:5])
    G = values[5]
    if isinstance(G, (bool, np.bool_)) or not isinstance(G, (int, float, np.integer, np.floating)):
        raise ValueError('watermark: strength must be a number, got {!r}'.format(G))
    if not 0 <= key < 2 ** 64:
        raise ValueError('watermark: key = {!r} is not in 0 .. 2^64 - 1'.format(key))
    if not 0 <= payload < 2 ** 32:
        raise ValueError('watermark: payload = {!r} is not in 0 .. 2^32 - 1'.format(payload))
    for name, v, lo, hi in (('payload_bits', P, 1, WM_BITS_MAX), ('chip', L, WM_CHIP_MIN, WM_CHIP_MAX), ('chips_per_symbol', C, 1, WM_SYMBOL_MAX)):
        if not lo <= v <= hi:
            raise ValueError('watermark: {} = {!r} is not in {} .. {}'.format(name, v, lo, hi))
        if name == 'chip' and v % 2:
            raise ValueError('watermark: chip = {!r} is not even'.format(v))
    if not 0.0 <= float(G) <= WM_STRENGTH_MAX:
        raise ValueError('watermark: strength = {!r} is not in 0 .. {:g}'.format(G, WM_STRENGTH_MAX))
    return (key, payload, P, L, C, float(G))


def watermark_zeta(score, energy, payload_bits):
    """the detection statistic of a record: (score - sqrt(2 P energy / pi)) / sqrt(energy (1 - 2 / pi)) -- with no mark every
    S[j] is about normal with variance energy / P, so the score is a sum of P half-normals of total variance energy.  0.0 where the
    energy is 0."""
    score, energy = float(score), float(energy)
    if energy <= 0.0:
        return 0.0
    return (score - math.sqrt(2.0 * payload_bits * energy / math.pi)) / math.sqrt(energy * (1.0 - 2.0 / math.pi))


# The delivery formats (TTS_FMT_* of include/sstts_hip.h) by the names every layer above uses, the numpy type of a code and the
# dither modes (TTS_DITHER_*)
FMT_F32, FMT_PCM_S16, FMT_PCM_U8, FMT_MULAW, FMT_ALAW = range(5)
FORMATS = {'float32': FMT_F32, 'pcm16': FMT_PCM_S16, 'pcm8': FMT_PCM_U8, 'mulaw': FMT_MULAW, 'alaw': FMT_ALAW}
FORMAT_NAMES = {v: k for k, v in FORMATS.items()}
FORMAT_DTYPES = {FMT_F32: np.float32, FMT_PCM_S16: np.int16, FMT_PCM_U8: np.uint8, FMT_MULAW: np.uint8, FMT_ALAW: np.uint8}
DITHER_NONE, DITHER_TPDF = 0, 1
ENCODE_TILE = 4096               # tts_encode_tile(), samples
OUTPUT_OFF = (FMT_F32, DITHER_NONE, 0, 0)   # the checked ``output`` of a call as it always was: float32 at the model's rate


def format_value(what, fmt, encoding=False):
    """a format -- one of the names of FORMATS or its TTS_FMT_* number -- as that number; ``encoding``: 'float32' is refused
    too.  ValueError, raised before a handle is touched."""
    if isinstance(fmt, str) and fmt in FORMATS:
        f = FORMATS[fmt]
    elif not isinstance(fmt, (bool, np.bool_, str)) and fmt in FORMAT_NAMES:
        f = int(fmt)
    else:
        raise ValueError('{}: the format must be one of {}, got {!r}'.format(what, ', '.join(sorted(FORMATS)), fmt))
    if encoding and f == FMT_F32:
        raise ValueError('{}: float32 is no encoding (the rows are float32 already)'.format(what))
    return f


def dither_value(what, dither):
    """``dither`` -- 'tpdf', True or TTS_DITHER_TPDF; None, False, 'none' or TTS_DITHER_NONE -- as TTS_DITHER_*; ValueError for
    anything else"""
    number = isinstance(dither, (int, np.integer)) and not isinstance(dither, (bool, np.bool_))
    if dither is None or dither is False or (isinstance(dither, str) and dither == 'none') or (number and dither == DITHER_NONE):
        return DITHER_NONE
    if dither is True or (isinstance(dither, str) and dither == 'tpdf') or (number and dither == DITHER_TPDF):
        return DITHER_TPDF
    raise ValueError("{}: dither must be 'tpdf' or None, got {!r}".format(what, dither))


def output_setting(output):
    """``output`` of ``synthesize_host`` and the layers above -- None (the handle's setting as it stands), a format name or
    ``(format, dither, rate_in, rate_out)`` (rates in Hz; both None: no resampling) -- as None or a checked tuple ``(format number,
    dither number, rate_in, rate_out)``; a bare name is dithered and keeps the rate, and whatever changes nothing of a call --
    'float32' with equal rates or none -- is ``OUTPUT_OFF``.  ValueError, raised before a handle is
    touched, for what tts_set_output refuses: an unknown format or dither, rates that are not positive integers or whose ratio
    lies outside [0.25, 4]."""
    if output is None:
        return None
    if isinstance(output, (tuple, list)):
        if len(output) != 4:
            raise ValueError('output must be None, a format name or (format, dither, rate_in, rate_out), got {!r}'.format(output))
        fmt, dither, rate_in, rate_out = output
    else:
        fmt, dither, rate_in, rate_out = output, 'tpdf', None, None
    f = format_value('output', fmt)
    d = DITHER_NONE if f == FMT_F32 else dither_value('output', dither)
    if (rate_in is None) != (rate_out is None):
        raise ValueError('output: both rates or neither, got {!r} and {!r}'.format(rate_in, rate_out))
    if rate_in is None or (rate_in == 0 and rate_out == 0 and not isinstance(rate_in, (bool, np.bool_))):   # (0, 0: the checked form)
        return (f, d, 0, 0) if f != FMT_F32 else OUTPUT_OFF
    for r in (rate_in, rate_out):
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer)) or r < 1 or r > 2 ** 31 - 1:
            raise ValueError('output: a rate must be a positive integer of Hz, got {!r}'.format(r))
    if rate_in != rate_out:
        resample_ratio_value(float(rate_out) / float(rate_in))
    elif f == FMT_F32:
        return OUTPUT_OFF
    return f, d, int(rate_in), int(rate_out)


def output_is_on(setting):
    """whether a checked ``output`` changes anything of a call: an encoding, or two different rates"""
    return setting is not None and tuple(setting) != OUTPUT_OFF


def output_ratio(setting):
    """rate_out / rate_in of a checked ``output``; 1.0 without resampling"""
    return float(setting[3]) / float(setting[2]) if setting is not None and setting[2] != setting[3] else 1.0


def alignment_stats_setting(alignment_stats):
    """``alignment_stats`` of the synthesis calls -- None (the handle's setting as it stands), False (off), True (on, pad id 0)
    or ``(enabled, pad_id)`` -- as None or a checked tuple ``(enabled, pad_id)``.  ValueError, raised before a handle is touched,
    for anything else: a bare number is neither a switch nor a pad id."""
    if alignment_stats is None:
        return None
    if isinstance(alignment_stats, (bool, np.bool_)):
        return (bool(alignment_stats), 0)
    if isinstance(alignment_stats, (tuple, list)) and len(alignment_stats) == 2:
        enabled, pad_id = alignment_stats
        if (isinstance(enabled, (bool, np.bool_)) and isinstance(pad_id, (int, np.integer)) and not isinstance(pad_id, (bool, np.bool_))
                and -2 ** 31 <= int(pad_id) < 2 ** 31):
            return (bool(enabled), int(pad_id))
    raise ValueError('alignment_stats must be None, a bool or (enabled, pad_id), got {!r}'.format(alignment_stats))


def alignment_lengths(lengths, B, hi, name, bound):
    """the ``n_sent`` / ``n_steps`` argument of an alignment_stats call as None or a contiguous int32 array of B lengths in
    1 .. ``hi``, checked as tts_alignment_stats checks them -- ValueError, raised before a handle is touched"""
    if lengths is None:
        return None
    n = np.asarray(lengths)
    if n.shape != (B,) or n.dtype.kind not in 'iu':
        raise ValueError('{}: {} integers are needed, got shape {} of {}'.format(name, B, n.shape, n.dtype))
    return _checked_lengths(n, hi, name, bound)


def token_times_jump(max_jump, what='token_times'):
    """``max_jump`` of a tts_token_times call -- the most tokens a decoder step may advance over -- as an int in 1 .. 15;
    ValueError, raised before a handle is touched, for anything else"""
    if isinstance(max_jump, (bool, np.bool_)) or not isinstance(max_jump, (int, np.integer)) or not 1 <= int(max_jump) <= TOKEN_TIMES_MAX_JUMP:
        raise ValueError('{}: max_jump must be an integer in 1 .. {}, got {!r}'.format(what, TOKEN_TIMES_MAX_JUMP, max_jump))
    return int(max_jump)


TOKEN_TIMES_OFF = (False, 0, 4)   # tts_set_token_times as a fresh handle has it; 4: untuned, four characters per decoder step


def token_times_setting(token_times):
    """``token_times`` of the synthesis calls -- None (the handle's setting as it stands), False (off), True (on, pad id 0,
    max_jump 4) or ``(enabled, pad_id, max_jump)`` -- as None or a checked tuple ``(enabled, pad_id, max_jump)``; ValueError, raised
    before a handle is touched, for anything else"""
    if token_times is None:
        return None
    if isinstance(token_times, (bool, np.bool_)):
        return (bool(token_times),) + TOKEN_TIMES_OFF[1:]
    if isinstance(token_times, (tuple, list)) and len(token_times) == 3:
        enabled, pad_id, max_jump = token_times
        if isinstance(enabled, (bool, np.bool_)) and isinstance(pad_id, (int, np.integer)) and not isinstance(pad_id, bool) and \
                -2 ** 31 <= int(pad_id) < 2 ** 31:
            return (bool(enabled), int(pad_id), token_times_jump(max_jump, 'token_times'))
    raise ValueError('token_times must be None, a bool or (enabled, pad_id, max_jump), got {!r}'.format(token_times))


JOIN_MAX_PIECES = 4096      # tts_join_max_pieces()
JOIN_MAX_FADE = 1 << 20     # tts_join_max_fade()
JOIN_MAX_SAMPLES = 1 << 33  # the most output samples G * N_out of a call


def join_fades(counts, fade):
    """f_p = min(fade, count[p] // 2) of every piece: the samples either edge fades over"""
    return np.minimum(np.int64(fade), np.asarray(counts, dtype=np.int64) // 2)


def join_list(pieces, groups, B, N, fade):
    """The edit list of a join on a batch (B, N) as ``(pieces, groups, G, n_out)``: ``pieces`` a contiguous int32 array (P, 4) of
    ``row, first, count, gap`` -- what tts_join_piece_t holds --, ``groups`` a contiguous int32 array (P,) (None: one group) and
    ``n_out`` the int64 lengths of the G groups.  Checked as tts_join_plan checks it, in its order -- ValueError, raised before a
    handle or the library is touched."""
    try:
        q = np.asarray(pieces)
    except (TypeError, ValueError):
        q = None
    if q is None or q.ndim != 2 or q.shape[1] != 4 or q.shape[0] < 1 or q.dtype.kind not in 'iu':
        raise ValueError('join: pieces must be (P, 4) integers (row, first, count, gap) with P >= 1, got {!r}'.format(
            None if q is None else (q.shape, q.dtype)))
    P = int(q.shape[0])
    if groups is None:
        g = np.zeros(P, dtype=np.int64)
    else:
        g = np.asarray(groups)
        if g.shape != (P,) or g.dtype.kind not in 'iu':
            raise ValueError('join: groups must be {} integers, got shape {} of {}'.format(P, g.shape, g.dtype))
    if isinstance(fade, (bool, np.bool_)) or not isinstance(fade, (int, np.integer)) or fade < 0:
        raise ValueError('join: fade must be an integer >= 0, got {!r}'.format(fade))
    if B < 1 or N < 1:
        raise ValueError('join: need B, N >= 1, got {}, {}'.format(B, N))
    if fade > JOIN_MAX_FADE:
        raise ValueError('join: fade = {} is larger than tts_join_max_fade() = {}'.format(fade, JOIN_MAX_FADE))
    if P > JOIN_MAX_PIECES:
        raise ValueError('join: {} pieces are more than tts_join_max_pieces() = {}'.format(P, JOIN_MAX_PIECES))
    q64, g64 = q.astype(np.int64), g.astype(np.int64)
    if np.abs(q64).max() >= 2 ** 31 or np.abs(g64).max() >= 2 ** 31:
        raise ValueError('join: the list must hold 32-bit integers')
    for p, (row, first, count, _gap) in enumerate(q64.tolist()):
        if not 0 <= row < B:
            raise ValueError('join: row[{}] = {} is not in 0 .. B - 1 = {}'.format(p, row, B - 1))
        if not 0 <= first < N:
            raise ValueError('join: first[{}] = {} is not in 0 .. N - 1 = {}'.format(p, first, N - 1))
        if not 1 <= count <= N - first:
            raise ValueError('join: count[{}] = {} is not in 1 .. N - first = {}'.format(p, count, N - first))
    gl = g64.tolist()
    if gl[0] != 0:
        raise ValueError('join: group[0] = {}: the groups start at 0'.format(gl[0]))
    for p in range(1, P):
        if gl[p] - gl[p - 1] not in (0, 1):
            raise ValueError('join: group[{}] = {} follows {}: the groups are non-decreasing and none is empty'.format(p, gl[p], gl[p - 1]))
    G = gl[-1] + 1
    f = join_fades(q64[:, 2], fade).tolist()
    n_out = np.zeros(G, dtype=np.int64)
    o = 0
    for p, (_row, _first, count, gap) in enumerate(q64.tolist()):
        if p + 1 == P or gl[p + 1] != gl[p]:
            n_out[gl[p]] = o + count
            o = 0
            continue
        room = min(f[p], f[p + 1])
        if gap < -room:
            raise ValueError('join: gap[{}] = {} overlaps more than min(f[{}], f[{}]) = {} samples'.format(p, gap, p, p + 1, room))
        o += count + gap
    return np.ascontiguousarray(q, dtype=np.int32), np.ascontiguousarray(g, dtype=np.int32), G, n_out


def stretch_frame_counts(n_frames, B, T):
    """The ``n_frames`` argument of a stretch call as a contiguous int32 array of B lengths in 1 .. T (None stays None: all
    T), checked as tts_stretch_magnitudes checks them -- ValueError, raised before a handle is touched."""
    if n_frames is None:
        return None
    nf = np.asarray(n_frames)
    if nf.shape != (B,):
        raise ValueError('n_frames: shape {} for a batch of {}'.format(nf.shape, B))
    if nf.dtype.kind not in 'iu':
        raise ValueError('n_frames must be integers, got {}'.format(nf.dtype))
    return _checked_lengths(nf, T, 'n_frames', 'T')


MAX_SEGMENTS = 4096                            # segments of a call of a segment-wise stage (csrc/segments.h)
SEGMENTS_PER_LAUNCH = 64                       # ... whose entries travel with one launch


def segment_launches(S):
    """launches of a segment-wise stage (the warp, the shift, the segment-wise resampler) on S segments"""
    return -(-int(S) // SEGMENTS_PER_LAUNCH)


def _segment_records(what, segments, dtype, name):
    """``segments`` -- an array of the record ``dtype`` (called ``name``), or rows of its fields without the ``reserved`` ones, which
    are 0 -- as a contiguous array (S,) of ``dtype``.  ValueError for anything that is not such a list or does not fit the record's
    fields: an int32 field takes a signed, a uint32 field an unsigned 32-bit integer, a float field a number."""
    if isinstance(segments, np.ndarray) and segments.dtype == dtype and segments.ndim == 1:
        return np.ascontiguousarray(segments)
    fields = [(f, dtype[f]) for f in dtype.names if f != 'reserved']
    ints = [f for f, t in fields if t.kind in 'iu']
    try:
        rows = [tuple(r) for r in segments]
    except TypeError:
        rows = None
    if rows is None or any(len(r) != len(fields) for r in rows):
        raise ValueError('{}: segments must be a {} array or rows ({})'.format(what, name, ', '.join(f for f, _t in fields)))
    out = np.zeros(len(rows), dtype=dtype)
    for s, r in enumerate(rows):
        if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not np.iinfo(t).min <= v <= np.iinfo(t).max
               for v, (_f, t) in zip(r, fields) if t.kind in 'iu'):
            raise ValueError('{}: segment {} must hold 32-bit integers {} and {}, got {!r}'.format(what, s, ', '.join(ints[:-1]), ints[-1], r))
        for v, (f, t) in zip(r, fields):
            if t.kind in 'iu':
                out[f][s] = int(v)
                continue
            try:
                out[f][s] = float(v)
            except (TypeError, ValueError):
                raise ValueError('{}: segment {} needs a number as its {}, got {!r}'.format(what, s, f, v))
    return out


def _segment_counts_check(what, S, B, max_name):
    """the counts of a segment list as every plan checks them (``max_name``: the stage's tts_*_max...() of the public header)"""
    if S > MAX_SEGMENTS:
        raise ValueError('{}: {} segments are more than {} = {}'.format(what, S, max_name, MAX_SEGMENTS))
    if B > S:
        raise ValueError('{}: {} rows of {} segments: no row is without a segment'.format(what, B, S))


def _segment_rows_check(what, rows, B):
    """the order of a segment list's rows as every plan checks it: from 0 to B - 1, never decreasing, none skipped"""
    if rows[0] != 0:
        raise ValueError('{}: row of segment 0 is {}: the rows start at 0'.format(what, rows[0]))
    for s in range(1, len(rows)):
        if rows[s] - rows[s - 1] not in (0, 1):
            raise ValueError('{}: row of segment {} is {} and follows {}: the rows are non-decreasing and none is without a segment'.format(
                what, s, rows[s], rows[s - 1]))
    if rows[-1] != B - 1:
        raise ValueError('{}: row of segment {} is {}: the last row is B - 1 = {}'.format(what, len(rows) - 1, rows[-1], B - 1))


WARP_MAX_SEGMENTS = MAX_SEGMENTS               # tts_warp_max_segments()
WARP_SEGMENTS_PER_LAUNCH = SEGMENTS_PER_LAUNCH
WARP_STEP_MIN, WARP_STEP_MAX = 16384, 262144   # the rates 0.25 .. 4 times 65536
WARP_GAIN_MAX = 16.0
WARP_MAX_T_OUT = 1 << 30


def warp_count(frames, step):
    """output frames of a speech segment: ceil(frames * 65536 / step), exact"""
    return -((-int(frames) << 16) // int(step))


warp_launches = segment_launches


def warp_segments(segments):
    """``segments`` -- a WARP_SEGMENT array, or rows ``(row, first, frames, pause, step, gain)`` -- as a contiguous WARP_SEGMENT
    array (S,).  ValueError for anything that is not such a list or does not fit the record's fields."""
    return _segment_records('warp', segments, WARP_SEGMENT, 'WARP_SEGMENT')


def warp_list(segments, B, T, n_frames=None):
    """The segment list of a warp on a batch (B, F, T) as ``(segments, n_frames, n_out, count)``: a contiguous WARP_SEGMENT array,
    the lengths as ``stretch_frame_counts`` makes them, the int64 lengths of the B output rows and the int64 output frames of
    every segment.  Checked as tts_warp_plan checks it, in its order -- ValueError, raised before a handle or the library is
    touched."""
    q = warp_segments(segments)
    S = int(q.shape[0])
    if B < 1 or T < 1 or S < 1:
        raise ValueError('warp: need B, T, S >= 1')
    _segment_counts_check('warp', S, B, 'tts_warp_max_segments()')
    nf = stretch_frame_counts(n_frames, B, T)
    _segment_rows_check('warp', q['row'].tolist(), B)
    n_out = np.zeros(B, dtype=np.int64)
    count = np.zeros(S, dtype=np.int64)
    for s, (row, first, frames, pause, step, gain) in enumerate(q.tolist()):
        if frames < 0 or pause < 0:
            raise ValueError('warp: segment {} has a negative length (frames {}, pause {})'.format(s, frames, pause))
        if frames > 0 and pause > 0:
            raise ValueError('warp: segment {} is both speech ({} frames) and a pause ({} frames)'.format(s, frames, pause))
        if frames == 0 and pause == 0:
            raise ValueError('warp: segment {} is neither speech nor a pause (frames and pause are 0)'.format(s))
        c = pause
        if frames > 0:
            n = T if nf is None else int(nf[row])
            if first < 0 or first + frames > n:
                raise ValueError('warp: segment {} reads frames {} .. {} of row {}, which has 0 .. {}'.format(s, first, first + frames - 1, row, n - 1))
            if not WARP_STEP_MIN <= step <= WARP_STEP_MAX:
                raise ValueError('warp: segment {} has step {}, which is not in {} .. {}'.format(s, step, WARP_STEP_MIN, WARP_STEP_MAX))
            if not 0.0 <= gain <= WARP_GAIN_MAX:   # (a NaN fails both comparisons)
                raise ValueError('warp: segment {} has a gain that is not finite or lies outside 0 .. 16'.format(s))
            c = warp_count(frames, step)
        count[s] = c
        n_out[row] += c
    return q, nf, n_out, count


SHIFT_MAX_SEGMENTS = MAX_SEGMENTS               # tts_shift_max_segments()
SHIFT_SEGMENTS_PER_LAUNCH = SEGMENTS_PER_LAUNCH
SHIFT_TILE = 8                                  # tts_shift_tile()
SHIFT_MAX_ORDER = 256                           # tts_shift_max_order()
SHIFT_N_MIN, SHIFT_N_MAX = 128, 2048            # F = N + 1 with N a power of two in this range
SHIFT_UNITY = 65536
SHIFT_STEP_MIN, SHIFT_STEP_MAX = 32768, 131072  # one octave either way
SHIFT_SEMITONES_MAX = 12.0


def shift_step(semitones):
    """The step of ``semitones`` for a SHIFT_SEGMENT: floor(65536 * 2 ** (-st / 12) + 0.5), source bins per output bin times 65536
    (+12 semitones: 32768, 0: 65536, -12: 131072).  ValueError for a shift that is not finite or lies outside -12 .. 12."""
    try:
        st = float(semitones)
    except (TypeError, ValueError):
        raise ValueError('shift: a number of semitones in [-12, 12] is needed, got {!r}'.format(semitones))
    if not -SHIFT_SEMITONES_MAX <= st <= SHIFT_SEMITONES_MAX:   # (a NaN fails both comparisons)
        raise ValueError('shift: the semitones must be finite and lie in [-12, 12], got {!r}'.format(semitones))
    return int(np.floor(65536.0 * np.exp2(-np.float64(st) / 12.0) + 0.5))


def shift_order(sampling_rate):
    """the default order of the envelope: max(8, int(0.0015 * sampling_rate)), 33 at 22 050 Hz (untuned)"""
    return max(8, int(0.0015 * float(sampling_rate)))


shift_launches = segment_launches

def shift_bins_n(F):
    """N of F = N + 1 bins where N is a power of two in 128 .. 2048, else 0"""
    N = int(F) - 1
    return N if SHIFT_N_MIN <= N <= SHIFT_N_MAX and N & (N - 1) == 0 else 0


def shift_segments(segments):
    """``segments`` -- a SHIFT_SEGMENT array, or rows ``(row, first, frames, pitch_step, formant_step)`` -- as a contiguous
    SHIFT_SEGMENT array (S,).  ValueError for anything that is not such a list or does not fit the record's fields."""
    return _segment_records('shift', segments, SHIFT_SEGMENT, 'SHIFT_SEGMENT')


def shift_list(segments, B, F, T, n_frames=None, order=33):
    """The segment list of a shift on a batch (B, F, T) as ``(segments, n_frames)``: a contiguous SHIFT_SEGMENT array and the
    lengths as ``stretch_frame_counts`` makes them.  Checked as tts_shift_plan checks it, in its order and its words -- ValueError,
    raised before a handle or the library is touched."""
    q = shift_segments(segments)
    S = int(q.shape[0])
    if B < 1 or T < 1 or S < 1:
        raise ValueError('shift: need B, T, S >= 1')
    N = shift_bins_n(F)
    if not N:
        raise ValueError('shift: F = {} is not 2^m + 1 with 2^m in {} .. {}'.format(F, SHIFT_N_MIN, SHIFT_N_MAX))
    order_max = min(SHIFT_MAX_ORDER, N // 2)
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or not 2 <= order <= order_max:
        raise ValueError('shift: order = {} is not in 2 .. {}'.format(order, order_max))
    _segment_counts_check('shift', S, B, 'tts_shift_max_segments()')
    nf = stretch_frame_counts(n_frames, B, T)
    _segment_rows_check('shift', q['row'].tolist(), B)
    prev_end, prev_row = 0, 0
    for s, (row, first, frames, reserved, pitch_step, formant_step) in enumerate(q.tolist()):
        if row != prev_row:
            prev_end, prev_row = 0, row
        if frames < 1:
            raise ValueError('shift: segment {} has {} frames: at least 1 is needed'.format(s, frames))
        n = T if nf is None else int(nf[row])
        if first < 0 or first + frames > n:
            raise ValueError('shift: segment {} covers frames {} .. {} of row {}, which has 0 .. {}'.format(s, first, first + frames - 1, row, n - 1))
        if first < prev_end:
            raise ValueError("shift: segment {} starts at frame {} of row {}, in front of its predecessor's end {}: the ranges of a row ascend "
                             'and do not overlap'.format(s, first, row, prev_end))
        if reserved != 0:
            raise ValueError('shift: segment {} has reserved = {}, which must be 0'.format(s, reserved))
        for name, step in (('pitch_step', pitch_step), ('formant_step', formant_step)):
            if not SHIFT_STEP_MIN <= step <= SHIFT_STEP_MAX:
                raise ValueError('shift: segment {} has {} {}, which is not in {} .. {}'.format(s, name, step, SHIFT_STEP_MIN, SHIFT_STEP_MAX))
        prev_end = first + frames
    return q, nf


RESAMPLE_RATIO_MIN, RESAMPLE_RATIO_MAX = 0.25, 4.0
PITCH_OCTAVES_MAX = 1.0


def resample_ratio_value(ratio):
    """``ratio`` (target rate / source rate) of the resampling calls as a checked float.  ValueError, raised before a handle is
    touched, for what tts_resample refuses: a ratio that is not finite or lies outside [0.25, 4]."""
    try:
        r = float(ratio)
    except (TypeError, ValueError):
        raise ValueError('the resampling ratio must be a number in [0.25, 4], got {!r}'.format(ratio))
    if not RESAMPLE_RATIO_MIN <= r <= RESAMPLE_RATIO_MAX:   # (a NaN fails both comparisons)
        raise ValueError('the resampling ratio must be finite and lie in [0.25, 4], got {!r}'.format(ratio))
    return r


def resampled_valid(n, ratio):
    """The samples resampy writes for ``n`` input samples: int(n * ratio), the product in double, truncated."""
    r = resample_ratio_value(ratio)
    if int(n) != n or n < 1:
        raise ValueError('resampled_valid: need n >= 1 samples, got {!r}'.format(n))
    return int(np.float64(int(n)) * np.float64(r))


def resampled_length(n, ratio):
    """tts_resampled_length on the host: ceil(n * ratio) in double, the length librosa.core.resample (fix=True) returns."""
    r = resample_ratio_value(ratio)
    if int(n) != n or n < 1:
        raise ValueError('resampled_length: need n >= 1 samples, got {!r}'.format(n))
    return int(np.ceil(np.float64(int(n)) * np.float64(r)))


RESAMPLE_SEGMENTS_MAX = MAX_SEGMENTS           # tts_resample_segments_max()
RESAMPLE_SEGMENTS_PER_LAUNCH = SEGMENTS_PER_LAUNCH
RESAMPLE_SEGMENTS_MAX_RATIOS = 16              # tts_resample_segments_max_ratios(): distinct ratios below 1 per call
RESAMPLE_SEGMENTS_MAX_N_OUT = 1 << 30


def resample_segment_count(samples, ratio):
    """output samples of a segment: ``samples`` for a copy (ratio 1.0 exactly), else int(samples * ratio), the product in double"""
    return int(samples) if ratio == 1.0 else int(np.float64(int(samples)) * np.float64(ratio))


def resample_segment_records(segments):
    """``segments`` -- a RESAMPLE_SEGMENT array, or rows ``(row, first, samples, ratio)`` -- as a contiguous RESAMPLE_SEGMENT
    array (S,).  ValueError for anything that is not such a list or does not fit the record's fields."""
    return _segment_records('resample_segments', segments, RESAMPLE_SEGMENT, 'RESAMPLE_SEGMENT')


def resample_segment_list(segments, B, n, n_samples=None):
    """The segment list of a segment-wise resampling of a batch (B, n) as ``(segments, n_samples, n_out, count)``: a contiguous
    RESAMPLE_SEGMENT array, the lengths as a contiguous int32 array (None: all n), the int64 lengths of the B output rows and the
    int64 output samples of every segment.  Checked as tts_resample_segments_plan checks it, in its order -- ValueError, raised
    before a handle or the library is touched."""
    q = resample_segment_records(segments)
    S = int(q.shape[0])
    if B < 1 or n < 1 or S < 1:
        raise ValueError('resample_segments: need B, n, S >= 1')
    _segment_counts_check('resample_segments', S, B, 'tts_resample_segments_max()')
    ns = _sample_lengths(n_samples, B, n)
    _segment_rows_check('resample_segments', q['row'].tolist(), B)
    n_out = np.zeros(B, dtype=np.int64)
    count = np.zeros(S, dtype=np.int64)
    below, extra_at = set(), None
    for s, (row, first, samples, reserved, ratio) in enumerate(q.tolist()):
        have = n if ns is None else int(ns[row])
        if samples < 1:
            raise ValueError('resample_segments: segment {} has {} samples: at least 1 is needed'.format(s, samples))
        if first < 0 or first + samples > have:
            raise ValueError('resample_segments: segment {} reads samples {} .. {} of row {}, which has 0 .. {}'.format(
                s, first, first + samples - 1, row, have - 1))
        if not RESAMPLE_RATIO_MIN <= ratio <= RESAMPLE_RATIO_MAX:   # (a NaN fails both comparisons)
            raise ValueError('resample_segments: segment {} has a ratio that is not finite or lies outside [0.25, 4]'.format(s))
        if reserved != 0:
            raise ValueError('resample_segments: segment {} has reserved = {}, which must be 0'.format(s, reserved))
        if ratio < 1.0 and ratio not in below:
            if len(below) < RESAMPLE_SEGMENTS_MAX_RATIOS:
                below.add(ratio)
            elif extra_at is None:
                extra_at = s
        count[s] = resample_segment_count(samples, ratio)
        n_out[row] += count[s]
    if extra_at is not None:
        raise ValueError('resample_segments: segment {} brings distinct ratio below 1 number {}: a call takes '
                         'tts_resample_segments_max_ratios() = {}'.format(extra_at, RESAMPLE_SEGMENTS_MAX_RATIOS + 1, RESAMPLE_SEGMENTS_MAX_RATIOS))
    return q, ns, n_out, count


def pitch_octaves_value(octaves):
    """``pitch`` of the synthesis calls, in octaves, as a checked float (None stays None: the handle's setting as it stands).
    ValueError, raised before a handle is touched, for what tts_set_pitch refuses: a shift that is not finite or beyond one
    octave either way."""
    if octaves is None:
        return None
    try:
        o = float(octaves)
    except (TypeError, ValueError):
        raise ValueError('pitch must be a number of octaves in [-1, 1], got {!r}'.format(octaves))
    if not -PITCH_OCTAVES_MAX <= o <= PITCH_OCTAVES_MAX:   # (a NaN fails both comparisons)
        raise ValueError('pitch must be finite and lie in [-1, 1] octaves, got {!r}'.format(octaves))
    return o


def pitch_semitones_value(semitones):
    """``--pitch SEMITONES`` as octaves (semitones / 12), checked as ``pitch_octaves_value`` checks them."""
    try:
        st = float(semitones)
    except (TypeError, ValueError):
        raise ValueError('pitch must be a number of semitones in [-12, 12], got {!r}'.format(semitones))
    if not -12.0 <= st <= 12.0:
        raise ValueError('pitch must be finite and lie in [-12, 12] semitones, got {!r}'.format(semitones))
    return st / 12.0


def synth_frame_counts(T, speaking_rate, octaves):
    """``(T_wav, T_gl)`` of a synthesis call of T frames at ``speaking_rate`` shifted by ``octaves``, as csrc/synth_plan.h has
    them: the waveform rows hold hop (T_wav - 1) samples, T_wav = stretched_frames(T, speaking_rate) -- the pitch changes no
    shape -- and Griffin-Lim reconstructs from T_gl = stretched_frames(T, speaking_rate * 2 ** -octaves) frames.  Rate 1.0 and
    pitch 0: (T, T).  ValueError where the product leaves [0.25, 4]."""
    eff = float(speaking_rate) * float(np.exp2(-np.float64(octaves)))
    if not SPEAKING_RATE_MIN <= eff <= SPEAKING_RATE_MAX:
        raise ValueError('speaking rate {} times 2 ** -{} octaves = {} is outside [0.25, 4]'.format(speaking_rate, octaves, eff))
    T_wav = int(T) if speaking_rate == 1.0 else stretched_frames(T, speaking_rate)
    return T_wav, T_wav if octaves == 0.0 else stretched_frames(T, eff)


def synth_lengths(n_frames, T, speaking_rate, octaves, min_frames):
    """``(reported, gl)``, int32 arrays: the lengths such a call reports for utterances of ``n_frames`` frames -- those of the
    call without pitch -- and the lengths its Griffin-Lim runs on.  An utterance has min(T_r, max(min_frames,
    stretched_frames(n, r))) frames at rate r in rows of T_r; at rate 1.0 its length is n untouched."""
    T_wav, T_gl = synth_frame_counts(T, speaking_rate, octaves)
    n = np.asarray(n_frames, dtype=np.int32)

    def at_rate(r, T_r):
        return np.array([min(T_r, max(min_frames, stretched_frames(int(v), r))) for v in n], np.int32)

    stretch = speaking_rate != 1.0 or octaves != 0.0
    gl = at_rate(float(speaking_rate) * float(np.exp2(-np.float64(octaves))), T_gl) if stretch else n
    if octaves == 0.0:
        return gl, gl
    return (at_rate(speaking_rate, T_wav) if speaking_rate != 1.0 else n), gl


def pitch_frames(T, speaking_rate, octaves):
    """The frames Griffin-Lim reconstructs from in a call of T frames at ``speaking_rate`` shifted by ``octaves`` -- the
    length of ``init_phase``'s last axis.  ValueError where the product of the rate and 2 ** -octaves leaves [0.25, 4]."""
    return synth_frame_counts(T, speaking_rate, octaves)[1]


def _padded_rows(spec, B, T, F, stride):
    """A host ``spec`` (B, T, F) as the (B, T, stride) float32 array that is uploaded for rows ``stride`` > F floats apart:
    the contiguous array ``spec`` is the view ``a[:, :, :F]`` of, as it is, or a copy with NaN in the padding columns."""
    base = spec.base if isinstance(spec, np.ndarray) else None
    if (isinstance(base, np.ndarray) and base.shape == (B, T, stride) and base.dtype == np.float32 and
            base.flags['C_CONTIGUOUS'] and spec.ctypes.data == base.ctypes.data):
        return base
    padded = np.full((B, T, stride), np.nan, dtype=np.float32)
    padded[:, :, :F] = spec
    return padded


def _strided_rows(what, spec, B, T, F, row_stride, width='F'):
    """Time-major rows ``spec`` (B, T, F) whose rows lie ``row_stride`` floats apart (None: F) as ``(what is uploaded, the
    stride)``: a device buffer as it is, a host array through :func:`_padded_rows`.  A stride below F is a ValueError in the name
    of ``what`` -- or, with ``what`` None, the library's to refuse."""
    stride = F if row_stride is None else int(row_stride)
    if what is not None and stride < F:
        raise ValueError('{}: row_stride {} < {} = {}'.format(what, stride, width, F))
    if not _is_device(spec) and stride > F:
        spec = _padded_rows(spec, B, T, F, stride)
    return spec, stride


# The per-call synthesis settings.  The handle holds each of them (tts_set_* / tts_set_option; the C ABI has no getters, so the
# engine mirrors them); ``Engine.synthesize`` and ``Engine.synthesize_host`` take them as keywords, ``Engine.griffin_lim``
# takes ``momentum`` and ``phase_init``.  None always means the handle's setting as it stands; any other value holds for that
# call alone (``Engine._settings``).  In the order they are checked and applied in:
#   ``momentum``: the fast Griffin-Lim momentum in [0, 1) (librosa's and torchaudio's ``momentum``; 0 = the reference's plain
#     loop) -- the ``gl_momentum`` option, off (0) unless ``set_option`` changed it.
#   ``stop_at_silence``: ``(threshold_db, keep_frames)`` -- end-of-speech stopping (tts_set_end_of_speech, off unless
#     ``set_end_of_speech`` changed it): every utterance is reconstructed from its frames up to the last one whose loudest bin is
#     above ``threshold_db``, plus ``keep_frames``; ``wav`` keeps its shape, row b holds hop (n_frames[b] - 1) samples followed by
#     zeros.  The result of a call made with stopping on carries ``n_frames``, the int32 host array of the B lengths;
#     ``synth_frames`` / ``wait_host_frames`` return them for any call.
#   ``speaking_rate``: a rate in [0.25, 4] (tts_set_speaking_rate, 1.0 unless ``set_speaking_rate`` changed it): the magnitudes
#     are time-stretched ahead of Griffin-Lim, ``wav`` is (B, hop (T' - 1)) and ``init_phase`` (B, F, T') with T' =
#     ``stretched_frames(T, rate)``; mel, alignments and linear keep their length T.
#   ``pitch``: a shift in [-1, 1] octaves (tts_set_pitch, 0 unless ``set_pitch`` changed it): the magnitudes are stretched by
#     rate * 2 ** -pitch, and the resampler takes Griffin-Lim's samples back to the length of the call without pitch.  No shape
#     and no reported length changes but ``init_phase``'s, which is (B, F, ``pitch_frames(T, rate, pitch)``).
#   ``phase_init``: how Griffin-Lim starts when ``init_phase`` is None -- 'random' (from ``seed``) or 'estimate' (phases
#     estimated from the call's own magnitudes, ``phase_estimate``: behind the stretch, at each utterance's own length; ``seed``
#     is then unused) -- the ``gl_init`` option.  An explicit ``init_phase`` always wins.
#   ``loudness``: a target in LUFS or ``(target_lufs, max_peak)`` (tts_set_loudness, off unless ``set_loudness`` changed it):
#     the call's final rows are taken to the target by ``loudness_normalize`` at the model's sampling rate, each utterance
#     over the samples its row holds, and ``peak_normalize`` is not applied.
#   ``alignment_stats``: False, True or ``(enabled, pad_id)`` (tts_set_alignment_stats, off unless ``set_alignment_stats``
#     changed it): the call also reduces its alignments to one record per utterance behind its decoder, with no host wait;
#     ``synth_alignment_stats(B)`` / ``wait_host_alignment_stats`` fetch them.  Nothing else of the call changes.
#   ``limiter``: a ceiling or ``(ceiling, lookahead_ms, oversample)`` (tts_set_limiter, off unless ``set_limiter`` changed it): the
#     call's final rows go through ``limit`` last, behind the loudness gain or the peak normalisation, each utterance over the
#     samples its row holds; the look-ahead is taken at the model's sampling rate.
#   ``output``: a format name or ``(format, dither, rate_in, rate_out)`` (tts_set_output, off unless ``set_output`` changed it):
#     ``synthesize_host`` alone -- the call's final rows are resampled and encoded on the device, behind the limiter, and only the
#     codes and their records travel to the host (``wait_host_encoded``).  ``synthesize`` refuses the keyword: it hands out device
#     rows, and ``encode`` is its callers' to call.
#   ``token_times``: False, True or ``(enabled, pad_id, max_jump)`` (tts_set_token_times, off unless ``set_token_times`` changed
#     it): the call also searches its alignments for the best monotone path behind its decoder, with no host wait;
#     ``synth_token_times(B)`` / ``wait_host_token_times`` fetch the step every token starts at.  Nothing else of the call changes.
#   ``watermark``: a key, ``(key, payload)`` or the full tuple of ``watermark_setting`` (tts_set_watermark, off unless
#     ``set_watermark`` changed it): the call's rows go through ``watermark_embed``.  The defaults are UNTUNED.
#   ``compressor``: a profile name of CMP_PROFILES or ``(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db)``
#     (tts_set_compressor, off unless ``set_compressor`` changed it): the call's rows go through ``compress``; the coefficients are
#     made at the model's sampling rate.
#   ``equalizer``: a profile name of EQ_PROFILES, a list of ``(kind, f0_hz, q, gain_db)`` sections or an (S, 5) array of sections
#     (tts_set_equalizer, off unless ``set_equalizer`` changed it): the call's rows go through ``equalize``; a design is made at the
#     model's sampling rate.  A boost behind the peak normalisation can pass 1.0: give it a limiter or a loudness target.
# The last three run in place behind Griffin-Lim, the pitch resampler and the peak normalisation -- the equaliser, then the
# compressor, then the watermark -- and ahead of the loudness gain and the limiter, each utterance over the samples its row holds.
# Lengths, shapes and timing marks do not change (the equaliser's group delay of a few samples is ignored).
# A row: the keyword, the Engine attribute that mirrors the handle's value, the handle's initial value, the check that turns
# the keyword into the mirror's value (ValueError before a handle is touched), how a value is applied -- a ``set_option``
# key or a call of the engine's ``set_*`` method -- and whether the keyword is the host form's alone.
Setting = collections.namedtuple('Setting', 'keyword mirror initial check apply host_only', defaults=(False,))
SETTINGS = (
    Setting('momentum', '_gl_momentum', 0, momentum_thousandths, 'gl_momentum'),
    Setting('stop_at_silence', '_end_of_speech', (False, 0.0, 0), lambda v: (True,) + stop_at_silence_setting(v),
            lambda engine, v: engine.set_end_of_speech(*v)),
    Setting('speaking_rate', '_speaking_rate', 1.0, speaking_rate_value, lambda engine, v: engine.set_speaking_rate(v)),
    Setting('pitch', '_pitch', 0.0, pitch_octaves_value, lambda engine, v: engine.set_pitch(v)),
    Setting('phase_init', '_gl_init', 0, phase_init_value, 'gl_init'),
    Setting('loudness', '_loudness', None, loudness_setting, lambda engine, v: engine.set_loudness(v)),
    Setting('alignment_stats', '_alignment_stats', (False, 0), alignment_stats_setting, lambda engine, v: engine.set_alignment_stats(*v)),
    Setting('limiter', '_limiter', None, limiter_setting, lambda engine, v: engine.set_limiter(v)),
    Setting('output', '_output', OUTPUT_OFF, output_setting, lambda engine, v: engine.set_output(v), host_only=True),
    Setting('token_times', '_token_times', TOKEN_TIMES_OFF, token_times_setting, lambda engine, v: engine.set_token_times(*v)),
    Setting('watermark', '_watermark', None, watermark_setting, lambda engine, v: engine.set_watermark(v)),
    Setting('compressor', '_compressor', None, compressor_setting, lambda engine, v: engine.set_compressor(v)),
    Setting('equalizer', '_equalizer', None, equalizer_setting, lambda engine, v: engine.set_equalizer(v)),
)


class _Settings(object):
    """The settings of one call: the ``per_call`` keywords of SETTINGS, every one checked here, in the table's order.  As a
    context manager it puts the handle to those that differ from it, in the table's order, and puts back afterwards, in reverse
    and also after an exception, those whose mirror no longer holds what it held.  ``self[keyword]``: the value the call runs
    with, in the mirror's form -- the keyword's, or the handle's as it stands."""

    def __init__(self, engine, per_call):
        self.engine = engine
        self.rows = [row for row in SETTINGS if row.keyword in per_call]
        self.values = {row.keyword: None if per_call[row.keyword] is None else row.check(per_call[row.keyword]) for row in self.rows}

    def __getitem__(self, keyword):
        if self.values[keyword] is not None:
            return self.values[keyword]
        return getattr(self.engine, next(row.mirror for row in self.rows if row.keyword == keyword))

    def _put(self, row, value):
        if getattr(self.engine, row.mirror) != value:
            self.engine.set_option(row.apply, value) if isinstance(row.apply, str) else row.apply(self.engine, value)

    def __enter__(self):
        with contextlib.ExitStack() as entered:
            for row in self.rows:
                saved = getattr(self.engine, row.mirror)
                if self.values[row.keyword] is not None:
                    self._put(row, self.values[row.keyword])
                entered.callback(self._put, row, saved)
            self.entered = entered.pop_all()
        return self

    def __exit__(self, *exc):
        return self.entered.__exit__(*exc)


class Engine(object):
    """One handle = one GPU + one stream.  Mirrors the C ABI one to one."""

    sampling_rate = 22050   # the model's (hparams.sampling_rate): what a loudness target of the synthesis calls is measured at

    def __init__(self, hparams=None, device_id=0, stream=None):
        self.lib = load_library()
        cfg = TtsConfig()
        self.lib.tts_default_config(byref(cfg))
        if hparams is not None:
            enc, dec, post = hparams.encoder, hparams.decoder, hparams.post
            cfg.vocabulary_size = hparams.vocabulary_size
            cfg.embedding_size = enc.embedding_size
            cfg.enc_prenet_units[0], cfg.enc_prenet_units[1] = [l[0] for l in enc.pre_net_layers]
            cfg.enc_n_banks, cfg.enc_n_filters = enc.n_banks, enc.n_filters
            cfg.enc_proj_filters[0], cfg.enc_proj_filters[1] = [p[0] for p in enc.projections]
            cfg.post_n_banks, cfg.post_n_filters = post.n_banks, post.n_filters
            cfg.post_proj_filters[0], cfg.post_proj_filters[1] = [p[0] for p in post.projections]
            cfg.n_highway_layers, cfg.n_highway_units = enc.n_highway_layers, enc.n_highway_units
            cfg.n_gru_units = enc.n_gru_units
            cfg.dec_prenet_units[0], cfg.dec_prenet_units[1] = [l[0] for l in dec.pre_net_layers]
            cfg.n_attention_units = dec.n_attention_units
            cfg.n_decoder_gru_units = dec.n_decoder_gru_units
            cfg.n_decoder_gru_layers = dec.n_gru_layers
            cfg.n_mels, cfg.reduction, cfg.n_fft = hparams.n_mels, hparams.reduction, hparams.n_fft
            cfg.force_cudnn = 1 if hparams.force_cudnn else 0
            att = hparams.attention
            if att.mechanism not in ('LuongAttention', 'LocalLuongAttention'):
                raise NotImplementedError('attention mechanism {!r}'.format(att.mechanism))
            if att.mechanism == 'LocalLuongAttention' and (att.luong_local_mode not in ('monotonic', 'predictive') or
                                                           att.luong_local_score != 'dot'):
                raise NotImplementedError('LocalLuongAttention: the general / concat scores raise '
                                          'NotImplementedError in the reference too')
            cfg.luong_local_mode = 1 if att.luong_local_mode == 'predictive' else 0
            cfg.attention_mechanism = 1 if att.mechanism == 'LocalLuongAttention' else 0
            cfg.luong_local_window_d = att.luong_local_window_D
            cfg.luong_force_gaussian = 1 if att.luong_force_gaussian else 0
            cfg.apply_post_processing = 1 if hparams.apply_post_processing else 0
            self.sampling_rate = int(getattr(hparams, 'sampling_rate', Engine.sampling_rate))
        self.cfg = cfg
        h = c_void_p()
        rc = self.lib.tts_create(byref(cfg), device_id, byref(h))
        if rc != TTS_OK:
            raise TtsError(rc, (self.lib.tts_last_error(None) or b'').decode())
        self.handle = h
        self.device_id = int(device_id)
        self._staging = {}
        self._init_settings()
        self._host_shapes, self._host_out_shapes = {}, {}   # per ticket of synthesize_host, until its wait_host* call
        if stream is not None:
            self._check(self.lib.tts_set_stream(self.handle, c_void_p(stream)))

    def set_stream(self, stream):
        """Adopt a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); None: a stream of the library's own."""
        self._check(self.lib.tts_set_stream(self.handle, c_void_p(stream) if stream else None))

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != TTS_OK:
            msg = (self.lib.tts_last_error(self.handle) or b'').decode()
            if rc == TTS_ERR_DB_RANGE:
                raise AssertionError(msg)   # reference audio/conversion.py:47-49
            raise TtsError(rc, msg)

    def _host_plan_check(self, rc):
        """``_check`` for a tts_*_plan call, which takes no handle: the text is tts_last_error(NULL)'s"""
        if rc != TTS_OK:
            raise TtsError(rc, (self.lib.tts_last_error(None) or b'').decode())

    def _check_or_free(self, rc, *outputs):
        """``_check`` for a call that enqueues nothing where it refuses: its fresh ``outputs`` (None among them) go back at once"""
        try:
            self._check(rc)
        except Exception:
            for a in outputs:
                if a is not None:
                    a.free()
            raise

    def close(self):
        if getattr(self, 'handle', None):
            for d in self._staging.values():
                d.free()
            self._staging = {}
            self.lib.tts_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._check(self.lib.tts_set_option(self.handle, key.encode(), int(value)))
        for row in SETTINGS:
            if row.apply == key:
                setattr(self, row.mirror, int(value))

    def _init_settings(self):
        """the mirrors of SETTINGS as a fresh handle has them; the ``set_*`` methods and ``set_option`` keep them"""
        for row in SETTINGS:
            setattr(self, row.mirror, row.initial)

    def _settings(self, **per_call):
        """the settings of one call (SETTINGS): checked here, applied around the ``with`` block"""
        return _Settings(self, per_call)

    def set_end_of_speech(self, enabled, threshold_db=0.0, keep_frames=0):
        """tts_set_end_of_speech: the handle's setting, read by every synthesize / synthesize_host call made after it."""
        self._check(self.lib.tts_set_end_of_speech(self.handle, 1 if enabled else 0, float(threshold_db), int(keep_frames)))
        self._end_of_speech = (bool(enabled), float(threshold_db), int(keep_frames))

    def set_speaking_rate(self, rate):
        """tts_set_speaking_rate: the handle's setting, read by every synthesize / synthesize_host call made after it;
        1.0 = off."""
        r = speaking_rate_value(rate)
        if r is None:
            raise ValueError('set_speaking_rate: a rate in [0.25, 4] is needed')
        self._check(self.lib.tts_set_speaking_rate(self.handle, r))
        self._speaking_rate = r

    def set_pitch(self, octaves):
        """tts_set_pitch: the handle's setting, read by every synthesize / synthesize_host call made after it; 0 = off."""
        o = pitch_octaves_value(octaves)
        if o is None:
            raise ValueError('set_pitch: a shift in [-1, 1] octaves is needed')
        self._check(self.lib.tts_set_pitch(self.handle, o))
        self._pitch = o

    def set_loudness(self, loudness, sampling_rate=None):
        """tts_set_loudness: the handle's setting, read by every synthesize / synthesize_host call made after it.  ``loudness``:
        None or False (off), a target in LUFS or ``(target_lufs, max_peak)``; measured at ``sampling_rate`` (None: the
        model's)."""
        setting = loudness_setting(None if loudness is False else loudness)
        if setting is None:
            self._check(self.lib.tts_set_loudness(self.handle, 0, 0.0, 1.0, 0))
        else:
            sr = loudness_sampling_rate('set_loudness', self.sampling_rate if sampling_rate is None else sampling_rate)
            self._check(self.lib.tts_set_loudness(self.handle, 1, setting[0], setting[1], sr))
        self._loudness = setting

    def set_limiter(self, limiter, sampling_rate=None):
        """tts_set_limiter: the handle's setting, read by every synthesize / synthesize_host call made after it.  ``limiter``:
        None or False (off), a ceiling or ``(ceiling, lookahead_ms, oversample)``; the look-ahead becomes samples at
        ``sampling_rate`` (None: the model's)."""
        setting = limiter_setting(None if limiter is False else limiter)
        if setting is None:
            self._check(self.lib.tts_set_limiter(self.handle, 0, 1.0, 0, 1))
        else:
            L = limiter_lookahead('set_limiter', setting[1], self.sampling_rate if sampling_rate is None else sampling_rate)
            self._check(self.lib.tts_set_limiter(self.handle, 1, setting[0], L, setting[2]))
        self._limiter = setting

    def set_equalizer(self, equalizer, sampling_rate=None):
        """tts_set_equalizer: the handle's setting, read by every synthesize / synthesize_host call made after it.  ``equalizer``:
        None or False (off), or what ``equalizer_setting`` reads -- a profile name, ``(kind, f0_hz, q, gain_db)`` sections or an
        (S, 5) array; a design is made at ``sampling_rate`` (None: the model's).  The library copies the sections."""
        setting = equalizer_setting(None if equalizer is False else equalizer)
        if setting is None:
            self._check(self.lib.tts_set_equalizer(self.handle, 0, None, 0))
        else:
            sos = equalizer_sections(setting, self.sampling_rate if sampling_rate is None else sampling_rate)
            self._check(self.lib.tts_set_equalizer(self.handle, 1, sos.ctypes.data_as(POINTER(ctypes.c_double)), len(sos)))
        self._equalizer = setting

    def set_compressor(self, compressor, sampling_rate=None):
        """tts_set_compressor: the handle's setting, read by every synthesize / synthesize_host call made after it.  ``compressor``:
        None or False (off), or what ``compressor_setting`` reads -- a profile name or ``(threshold_db, ratio, knee_db, attack_ms,
        release_ms, makeup_db)``; the coefficients are made at ``sampling_rate`` (None: the model's).  The library copies them."""
        setting = compressor_setting(None if compressor is False else compressor)
        if setting is None:
            self._check(self.lib.tts_set_compressor(self.handle, 0, None))
        else:
            p = TtsCompressor(*compressor_params(setting, self.sampling_rate if sampling_rate is None else sampling_rate))
            self._check(self.lib.tts_set_compressor(self.handle, 1, ctypes.addressof(p)))
        self._compressor = setting

    def set_watermark(self, watermark):
        """tts_set_watermark: the handle's setting, read by every synthesize / synthesize_host call made after it.  ``watermark``:
        None or False (off), or what ``watermark_setting`` reads -- a key, ``(key, payload)`` or ``(key, payload, payload_bits, chip,
        chips_per_symbol, strength)``.  The library copies the parameters.  The defaults are UNTUNED."""
        setting = watermark_setting(None if watermark is False else watermark)
        if setting is None:
            self._check(self.lib.tts_set_watermark(self.handle, 0, None))
        else:
            p = TtsWatermark(*setting)
            self._check(self.lib.tts_set_watermark(self.handle, 1, ctypes.addressof(p)))
        self._watermark = setting

    def set_output(self, output):
        """tts_set_output: the handle's setting, read by every synthesize_host call made after it.  ``output``: None, False or
        'float32' (off), a format name ('pcm16', 'pcm8', 'mulaw', 'alaw': TPDF dither, the model's rate) or ``(format, dither,
        rate_in, rate_out)`` as ``output_setting`` reads it."""
        setting = OUTPUT_OFF if output is None or output is False else output_setting(output)
        self._check(self.lib.tts_set_output(self.handle, *setting))
        self._output = setting

    def set_alignment_stats(self, enabled, pad_id=0):
        """tts_set_alignment_stats: the handle's setting, read by every synthesize / synthesize_host call made after it.  On,
        every call also reduces its alignments to one record per utterance (``alignment_stats``), the sentence lengths taken
        from its ids with ``pad_id`` as the padding (``text_lengths``): ``synth_alignment_stats`` /
        ``wait_host_alignment_stats`` fetch them."""
        setting = alignment_stats_setting((bool(enabled), pad_id))
        self._check(self.lib.tts_set_alignment_stats(self.handle, 1 if setting[0] else 0, setting[1]))
        self._alignment_stats = setting

    def synchronize(self):
        self._check(self.lib.tts_synchronize(self.handle))

    def empty(self, shape, dtype=np.float32):
        return DeviceArray(self, shape, dtype)

    def to_device(self, host, dtype=None):
        host = np.asarray(host)
        return DeviceArray(self, host.shape, dtype or host.dtype).copy_from(host)

    def _in(self, x, dtype, role=None):
        """-> (pointer, keepalive) for a host array or a device buffer.

        Host arrays are uploaded with tts_memcpy_h2d, which waits for the handle's stream: a call fed from
        host memory therefore starts after the previous call's Griffin-Lim has finished, i.e. the stream
        pipelining of tts_synthesize only overlaps calls whose inputs are device resident.  With a `role`
        the staging buffer is kept and reused by later calls of the same size (a fresh buffer per call
        would add a hipFree, which synchronises the whole device)."""
        if x is None:
            return None, None
        if _is_device(x):
            return x.data_ptr(), x
        host = np.ascontiguousarray(x, dtype=dtype)
        if role is None:
            d = self.to_device(host, dtype)
            return d.ptr, d
        d = self._staging.get(role)
        if d is None or d.nbytes != host.nbytes:
            if d is not None:
                d.free()
            d = DeviceArray(self, host.shape, dtype)
            self._staging[role] = d
        d.shape = host.shape
        d.copy_from(host)
        return d.ptr, d

    def _check_ids(self, ids):
        """tf.nn.embedding_lookup on the CPU raises for ids outside the table (reference
        tacotron/model.py:154); device-resident ids cannot be inspected without a synchronisation, the
        kernel reads them as a zero row (TF's GPU behaviour)."""
        if isinstance(ids, np.ndarray) and ids.size:
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.cfg.vocabulary_size:
                raise TtsError(TTS_ERR_INVALID, 'sentence ids must lie in [0, {}): got [{}, {}]'.format(
                    self.cfg.vocabulary_size, lo, hi))

    # ------------------------------------------------------------------ weights
    def manifest(self):
        out = []
        n = self.lib.tts_manifest_size(self.handle)
        for i in range(n):
            name = c_char_p()
            shape = (c_int64 * 4)()
            nd = c_int()
            self._check(self.lib.tts_manifest_entry(self.handle, i, byref(name), shape, byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[d]) for d in range(nd.value))))
        return out

    def load_weights(self, weights):
        """weights: {tf variable name: array in TensorFlow layout}."""
        for name, shape in self.manifest():
            if name not in weights:
                raise TtsError(TTS_ERR_NOT_LOADED, 'missing weight ' + name)
            w = np.ascontiguousarray(weights[name], dtype=np.float32)
            shp = (c_int64 * max(1, w.ndim))(*w.shape)
            self._check(self.lib.tts_set_weight(self.handle, name.encode(), w.ctypes.data, shp, w.ndim))
        self._check(self.lib.tts_finalize_weights(self.handle))

    def load_weights_blob(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
        self._check(self.lib.tts_load_weights_blob(self.handle, blob.ctypes.data, blob.size))
        self._check(self.lib.tts_finalize_weights(self.handle))

    # ------------------------------------------------------------------ stages
    def encoder_forward(self, ids, out=None):
        B, Ts = ids.shape
        self._check_ids(ids)
        p_ids, _k = self._in(ids, np.int32, 'ids')
        mem = out if out is not None else self.empty((B, Ts, 2 * self.cfg.n_gru_units))
        self._check(self.lib.tts_encoder_forward(self.handle, p_ids, B, Ts, mem.data_ptr()))
        return mem

    def decoder_forward(self, memory, n_steps, want_alignments=True, mel=None, alignments=None):
        B, Ts = memory.shape[0], memory.shape[1]
        p_mem, _k = self._in(memory, np.float32)
        if mel is None:
            mel = self.empty((B, n_steps, self.cfg.reduction * self.cfg.n_mels))
        if alignments is None and want_alignments:
            alignments = self.empty((n_steps, B, Ts))
        self._check(self.lib.tts_decoder_forward(self.handle, p_mem, B, Ts, n_steps, mel.data_ptr(),
                                                 alignments.data_ptr() if alignments is not None else None))
        return mel, alignments

    def postnet_forward(self, mel, out=None):
        B, T = mel.shape[0], mel.shape[1]
        p_mel, _k = self._in(mel, np.float32)
        lin = out if out is not None else self.empty((B, T, 1 + self.cfg.n_fft // 2))
        self._check(self.lib.tts_postnet_forward(self.handle, p_mel, B, T, lin.data_ptr()))
        return lin

    def evaluate(self, ids, mel_target, linear_target, want_sums=False, want_mel=False, want_alignments=False,
                 want_linear=False, losses=None):
        """Mode.EVAL on one batch (tts_evaluate): ids int32 (B, T_sent), targets as the reference feeds them --
        mel (B, T_red, r*n_mels) or (B, T, n_mels), linear (B, T_red, r*F) or (B, T, F), zero-padded -- host arrays or
        device buffers.  The decoder free-runs for n_steps = T_red.  Returns a dict with the device arrays ``losses``
        (3,) = [loss, loss_decoder, loss_post_processing] and, where asked for, ``l1_sums`` (B, 2) float64, ``mel``
        (B, T, n_mels), ``alignments`` (T_red, B, T_sent), ``linear`` (B, T, F)."""
        return self._with_targets(False, ids, mel_target, linear_target, want_sums, want_mel, want_alignments, want_linear, losses)

    def _teacher_steps(self, mel_target, B, what, empty_ok=False):
        r, nm = self.cfg.reduction, self.cfg.n_mels
        mel_sz = int(np.prod(mel_target.shape))
        if mel_target.shape[0] != B or (mel_sz == 0 and not empty_ok) or mel_sz % (B * r * nm):
            raise ValueError('{}: mel target of shape {} for B = {}, r * n_mels = {}'.format(what, mel_target.shape, B, r * nm))
        return mel_sz // (B * r * nm)

    def decoder_forward_teacher(self, memory, mel_target, want_alignments=True, mel=None, alignments=None):
        """Teacher-forced decoder (tts_decoder_forward_teacher; reference helpers.py:208-405, TacotronTrainingHelper):
        step 0 reads the GO frame, step t >= 1 frame t*r - 1 of ``mel_target`` -- (B, S, r*n_mels) or (B, S*r, n_mels), host
        array or device buffer; n_steps = S.  The inference network otherwise (no dropout, moving batch-norm statistics, no
        gradient): this is not Mode.TRAIN.  Returns (mel (B, S, r*n_mels), alignments (S, B, Ts) or None), as
        :meth:`decoder_forward`."""
        B, Ts = memory.shape[0], memory.shape[1]
        n_steps = self._teacher_steps(mel_target, B, 'decoder_forward_teacher')
        p_mem, _k1 = self._in(memory, np.float32)
        p_tgt, _k2 = self._in(mel_target, np.float32, 'teacher_mel_target')
        if mel is None:
            mel = self.empty((B, n_steps, self.cfg.reduction * self.cfg.n_mels))
        if alignments is None and want_alignments:
            alignments = self.empty((n_steps, B, Ts))
        self._check(self.lib.tts_decoder_forward_teacher(self.handle, p_mem, B, Ts, n_steps, p_tgt, mel.data_ptr(),
                                                         alignments.data_ptr() if alignments is not None else None))
        return mel, alignments

    def teacher_forced(self, ids, mel_target, linear_target=None, want_sums=False, want_mel=True, want_alignments=True,
                       want_linear=True, losses=None):
        """Teacher-forced forward pass on one batch (tts_teacher_forced): encoder, the decoder of
        :meth:`decoder_forward_teacher`, the post-net on its mel prediction and -- with ``linear_target`` -- the L1 losses
        of :meth:`evaluate`.  Shapes and inputs as :meth:`evaluate` takes them; no dropout, no batch statistics, no
        gradient (not Mode.TRAIN).  Returns a dict of device arrays: ``mel`` (B, T, n_mels), ``alignments``
        (T_red, B, T_sent), ``linear`` (B, T, F) where asked for, ``losses`` (3,) and ``l1_sums`` (B, 2) float64 (with
        ``want_sums``) when a linear target is given, else None; and ``n_steps``."""
        return self._with_targets(True, ids, mel_target, linear_target, want_sums, want_mel, want_alignments, want_linear, losses)

    def _with_targets(self, teacher, ids, mel_target, linear_target, want_sums, want_mel, want_alignments, want_linear, losses):
        """:meth:`evaluate` (the decoder free-runs, both targets are required and losses always come back) and
        :meth:`teacher_forced` (the decoder reads ``mel_target``; losses with a ``linear_target`` alone)"""
        what = 'teacher_forced' if teacher else 'evaluate'
        B, Ts = ids.shape
        r, nm, F = self.cfg.reduction, self.cfg.n_mels, 1 + self.cfg.n_fft // 2
        n_steps = self._teacher_steps(mel_target, B, what, empty_ok=not teacher)
        T = n_steps * r
        with_losses = linear_target is not None or not teacher
        if with_losses and (linear_target.shape[0] != B or int(np.prod(linear_target.shape)) != B * T * F):
            raise ValueError('{}: linear target of shape {}, ({}, {}, {}) floats needed'.format(what, linear_target.shape, B, T, F))
        self._check_ids(ids)
        role = 'teacher' if teacher else 'eval'
        p_ids, _k1 = self._in(ids, np.int32, 'ids')
        p_mel, _k2 = self._in(mel_target, np.float32, role + '_mel_target')
        p_lin, _k3 = self._in(linear_target, np.float32, role + '_linear_target')
        out = dict(losses=(losses if losses is not None else self.empty((3,))) if with_losses else None)
        out['l1_sums'] = self.empty((B, 2), np.float64) if want_sums and with_losses else None
        out['mel'] = self.empty((B, T, nm)) if want_mel else None
        out['alignments'] = self.empty((n_steps, B, Ts)) if want_alignments else None
        out['linear'] = self.empty((B, T, F)) if want_linear else None
        ptr = lambda a: a.data_ptr() if a is not None else None
        call = self.lib.tts_teacher_forced if teacher else self.lib.tts_evaluate
        self._check(call(self.handle, p_ids, B, Ts, n_steps, p_mel, p_lin, ptr(out['losses']), ptr(out['l1_sums']), ptr(out['mel']),
                         ptr(out['alignments']), ptr(out['linear'])))
        out['n_steps'] = n_steps
        return out

    def teacher_kernel_choice(self, B, Ts):
        """tts_teacher_kernel_choice: 2 = decoder_ws.hip's teacher variant, 0 = launch per layer."""
        rc = self.lib.tts_teacher_kernel_choice(self.handle, int(B), int(Ts))
        if rc < 0:
            self._check(rc)
        return rc

    def denorm_power(self, linear, ref_db, max_db, power, out=None):
        B, T, F = linear.shape
        p_lin, _k = self._in(linear, np.float32)
        mag = out if out is not None else self.empty((B, F, T))
        self._check(self.lib.tts_denorm_power(self.handle, p_lin, B, T, F, ref_db, max_db, power, mag.data_ptr()))
        return mag

    def griffin_lim(self, mag, n_iter, win_length, hop_length, n_fft, init_phase=None, seed=0, want_mse=True, momentum=None,
                    n_frames=None, phase_init=None):
        """``momentum`` and ``phase_init``: for this call, as SETTINGS has them.
        ``n_frames``: B frame counts -- a ragged batch (tts_griffin_lim_ragged): ``mag`` and ``init_phase`` are padded to
        (B, F, T_max), utterance b is reconstructed from its first n_frames[b] columns alone (the padding never reaches a
        result), row b of ``wav`` holds its hop (n_frames[b] - 1) samples followed by zeros and ``mse[b]`` is its own."""
        call = self._settings(momentum=momentum, phase_init=phase_init)
        B, F, T = mag.shape
        nf = ragged_frame_counts(n_frames, B, T, hop_length, n_fft) if n_frames is not None else None
        p_mag, _k1 = self._in(mag, np.float32)
        p_init, _k2 = self._in(init_phase, np.float32)
        wav = self.empty((B, hop_length * (T - 1)))
        mse = self.empty((B,)) if want_mse else None
        if nf is not None:
            with call:
                self._check(self.lib.tts_griffin_lim_ragged(self.handle, p_mag, p_init, seed, B, T, _int32_ptr(nf),
                                                            n_iter, win_length, hop_length, n_fft, wav.data_ptr(),
                                                            mse.data_ptr() if mse is not None else None))
            return wav, mse
        with call:
            self._check(self.lib.tts_griffin_lim(self.handle, p_mag, p_init, seed, B, T, n_iter, win_length, hop_length,
                                                 n_fft, wav.data_ptr(), mse.data_ptr() if mse is not None else None))
        return wav, mse

    # ------------------------------------------------------------------ estimated initial phases
    def phase_chunk_frames(self):
        """tts_phase_chunk_frames: the frames of one chunk of the estimate's cut in time (no result depends on it)."""
        return int(self.lib.tts_phase_chunk_frames())

    def phase_estimate(self, mag, n_fft, hop_length, n_frames=None):
        """tts_phase_estimate: initial phases for Griffin-Lim estimated from the magnitudes alone -- spectral peaks tracked
        from frame to frame, every other bin locked to the peak that owns it (include/sstts_hip.h has the definition,
        tests/phase_oracle.py restates it).  ``mag`` (B, F, T), the layout of ``griffin_lim`` -- a host array or a device
        buffer.  ``n_frames``: B lengths (host integers) -- columns at or behind them are neither read nor written; None: all T.
        Returns a device array (B, F, T) of numbers in [0, 1), the format of ``init_phase``."""
        B, T, F, nf = phase_estimate_args(mag.shape, n_fft, hop_length, n_frames)
        p_mag, _k = self._in(mag, np.float32)
        out = self.empty((B, F, T))
        self._check_or_free(self.lib.tts_phase_estimate(self.handle, p_mag, B, T, _int32_ptr(nf), int(n_fft), int(hop_length), out.data_ptr()), out)
        return out

    def phase_estimate_rows(self, spec, n_fft, hop_length, n_frames=None, row_stride=None):
        """tts_phase_estimate_rows: the same estimate from time-major rows, ``spec`` (B, T, F) as ``speech_frames`` takes it
        (``row_stride`` as there).  Returns the same device array (B, F, T) as :meth:`phase_estimate`."""
        B, T, F, nf = phase_estimate_args(spec.shape, n_fft, hop_length, n_frames, time_major=True)
        spec, stride = _strided_rows('phase_estimate_rows', spec, B, T, F, row_stride)
        p_spec, _k = self._in(spec, np.float32)
        out = self.empty((B, F, T))
        self._check_or_free(self.lib.tts_phase_estimate_rows(self.handle, p_spec, B, T, stride, _int32_ptr(nf), int(n_fft), int(hop_length),
                                                             out.data_ptr()), out)
        return out

    def peak_normalize(self, wav):
        B, n = wav.shape
        self._check(self.lib.tts_peak_normalize(self.handle, wav.data_ptr(), B, n))
        return wav

    def speech_threshold(self, threshold_db, ref_db, max_db, power=None):
        """tts_speech_threshold: ``threshold_db`` in the units of a spectrogram buffer, computed in double and rounded once
        to float32.  ``power`` None: normalised dB, the units of the network's ``linear`` -- (threshold_db - ref_db) /
        (|ref_db| + |max_db|) + 1; otherwise the units of the de-normalised magnitudes ** power --
        pow(pow(10, threshold_db / 20), power)."""
        out = c_float()
        rc = self.lib.tts_speech_threshold(float(threshold_db), float(ref_db), float(max_db),
                                           1.0 if power is None else float(power), 0 if power is None else 1, byref(out))
        if rc != TTS_OK:
            raise ValueError('speech_threshold({!r}, {!r}, {!r}, {!r}): a NaN, a zero dB range or power <= 0'.format(
                threshold_db, ref_db, max_db, power))
        return np.float32(out.value)

    def speech_frames(self, spec, threshold, keep_frames=0, min_frames=1, row_stride=None):
        """tts_speech_frames on ``spec`` (B, T, F), time-major -- a host array or a device buffer.  ``row_stride`` (>= F):
        the rows of the buffer are that many floats apart and only the first F of each are data.  A device buffer is then
        B * T * row_stride floats of which (B, T, F) is the logical shape; a host array may be the view ``a[:, :, :F]`` of a
        contiguous (B, T, row_stride) float32 array, which is uploaded as it is, padding included -- any other host array is
        uploaded with NaN in the padding columns (they never reach a result).

        Returns device int32 arrays ``(n_frames, last_active)`` of B entries: frame t is active iff np.max(spec[b, t]) >
        ``threshold`` (strict; a row that holds a NaN is silent), last_active = the last active frame or -1, n_frames =
        min(T, max(min_frames, last_active + 1 + keep_frames)).  ``threshold`` is in the units of ``spec``
        (:meth:`speech_threshold`)."""
        if len(spec.shape) != 3:
            raise ValueError('speech_frames: spec must be (B, T, F), got shape {}'.format(tuple(spec.shape)))
        B, T, F = (int(d) for d in spec.shape)
        spec, stride = _strided_rows(None, spec, B, T, F, row_stride)   # (a stride below F: the library refuses it)
        p_spec, _k = self._in(spec, np.float32)
        n_frames = self.empty((max(B, 1),), np.int32)
        last = self.empty((max(B, 1),), np.int32)
        self._check_or_free(self.lib.tts_speech_frames(self.handle, p_spec, B, T, F, stride, float(threshold), int(keep_frames), int(min_frames),
                                                       n_frames.data_ptr(), last.data_ptr()), n_frames, last)
        return n_frames, last

    def speech_interval(self, spec, threshold, row_stride=None):
        """tts_speech_interval: both ends of the reference's ``silence_interval_from_spectrogram`` on ``spec`` (B, T, F),
        time-major, a host array or a device buffer, with ``row_stride`` as in :meth:`speech_frames`.  Returns device int32
        arrays ``(first_active, last_active)`` of B entries: the first and the last frame t with np.max(spec[b, t]) >
        ``threshold`` (strict; a row that holds a NaN is silent), both -1 where no frame is active.  ``last_active`` is what
        :meth:`speech_frames` reports."""
        if len(spec.shape) != 3 or min(spec.shape) < 1:
            raise ValueError('speech_interval: spec must be a non-empty (B, T, F), got shape {}'.format(tuple(spec.shape)))
        B, T, F = (int(d) for d in spec.shape)
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError('speech_interval: the threshold is NaN')
        spec, stride = _strided_rows('speech_interval', spec, B, T, F, row_stride)
        p_spec, _k = self._in(spec, np.float32)
        first, last = self.empty((B,), np.int32), self.empty((B,), np.int32)
        self._check_or_free(self.lib.tts_speech_interval(self.handle, p_spec, B, T, F, stride, threshold, first.data_ptr(), last.data_ptr()),
                            first, last)
        return first, last

    # ------------------------------------------------------------------ the join
    def join_max_pieces(self):
        """tts_join_max_pieces: the most pieces :meth:`join` takes in one call."""
        return int(self.lib.tts_join_max_pieces())

    def join_max_fade(self):
        """tts_join_max_fade: the longest fade of :meth:`join`, in samples."""
        return int(self.lib.tts_join_max_fade())

    def join_tile(self):
        """tts_join_tile: the output samples one workgroup of the join writes."""
        return int(self.lib.tts_join_tile())

    def join_plan(self, shape, pieces, groups=None, fade=0):
        """tts_join_plan, host only: the lengths ``n_out`` (int64 (G,)) of the groups that ``pieces`` -- (P, 4) integers ``row,
        first, count, gap`` -- and ``groups`` (P integers, non-decreasing from 0, None: one group) make of a batch of ``shape``
        (B, N).  ValueError for a list tts_join refuses (``join_list``), raised before the library is reached."""
        if len(shape) != 2:
            raise ValueError('join_plan: the shape of a batch (B, N) is needed, got {!r}'.format(tuple(shape)))
        B, N = int(shape[0]), int(shape[1])
        q, g, G, n_out = join_list(pieces, groups, B, N, fade)
        out = np.zeros(G, dtype=np.int64)
        rc = self.lib.tts_join_plan(q.ctypes.data, q.shape[0], _int32_ptr(g), G, B, N, int(fade), out.ctypes.data_as(POINTER(c_int64)))
        self._host_plan_check(rc)
        assert (out == n_out).all(), (out, n_out)
        return out

    def join(self, wavs, pieces, groups=None, fade=0, N_out=None):
        """tts_join: pieces of the rows of ``wavs`` (B, N) -- a host array, which is uploaded, or a device buffer, which is read in
        place -- laid one behind the other into G output rows.  ``pieces``: (P, 4) integers ``row, first, count, gap`` -- samples
        [first, first + count) of a row, and the pause behind the piece in samples (negative: a cross-fade of that many samples
        with the next piece, at most min(f_p, f_p+1)); ``groups``: the output row of every piece, non-decreasing from 0 (None: one
        row); ``fade``: the samples either edge of a piece fades over (f_p = min(fade, count // 2)).  include/sstts_hip.h has the
        definition: the bits of tests/join_oracle.py.

        Returns ``(out, n_out)``: a fresh device array (G, N_out) and the int64 host lengths (G,) -- row g holds n_out[g] samples
        followed by +0.0.  ``N_out`` None: the largest length rounded up to a multiple of 4 (rows that start on a 16-byte
        boundary); otherwise at least the largest length.  ValueError for what the library refuses, raised before it is reached."""
        if len(wavs.shape) != 2 or min(wavs.shape) < 1:
            raise ValueError('join: a batch (B, N) is needed, got shape {}'.format(tuple(wavs.shape)))
        B, N = (int(d) for d in wavs.shape)
        q, g, G, n_out = join_list(pieces, groups, B, N, fade)
        longest = int(n_out.max())
        if N_out is None:
            N_out = (longest + 3) // 4 * 4
        if int(N_out) != N_out or not longest <= N_out < 2 ** 31:
            raise ValueError('join: N_out = {!r} is not in n_out.max() = {} .. 2^31 - 1'.format(N_out, longest))
        if G * int(N_out) > JOIN_MAX_SAMPLES:
            raise ValueError('join: G * N_out = {} output samples are more than 2^33 = {}'.format(G * int(N_out), JOIN_MAX_SAMPLES))
        p_wav, _k = self._in(wavs, np.float32)
        out = self.empty((G, int(N_out)))
        self._check_or_free(self.lib.tts_join(self.handle, p_wav, B, N, q.ctypes.data, q.shape[0], _int32_ptr(g), G, int(fade), int(N_out),
                                              out.data_ptr()), out)
        return out, n_out

    def download_rows(self, rows, lengths):
        """the first ``lengths[g]`` elements of every row of the device array ``rows`` (G, N) as a list of host arrays: only
        those bytes cross to the host (``to_host`` would bring all G * N)"""
        G, N = rows.shape
        lengths = [int(n) for n in lengths]
        if len(lengths) != G or any(not 0 <= n <= N for n in lengths):
            raise ValueError('download_rows: {} lengths in 0 .. {} are needed, got {!r}'.format(G, N, lengths))
        out = []
        for g, n in enumerate(lengths):
            host = np.empty(n, dtype=rows.dtype)
            if n:
                self._check(self.lib.tts_memcpy_d2h(self.handle, host.ctypes.data, rows.data_ptr() + g * N * rows.dtype.itemsize,
                                                    n * rows.dtype.itemsize))
            out.append(host)
        return out

    # ------------------------------------------------------------------ cepstra and alignment
    def mfcc(self, rows, n_mfcc, n_frames=None, clip01=False, row_stride=None):
        """tts_mfcc: the orthonormal DCT-II of ``rows`` (B, T, n_mels) along the mel axis, first ``n_mfcc`` coefficients -- the
        reference's calculate_mfccs (audio/features.py:89-113) on time-major rows, a host array or a device buffer
        (``row_stride`` as :meth:`speech_frames` takes it).  ``clip01``: np.clip(rows, 0, 1) first.  ``n_frames``: B lengths
        (host integers); rows at or behind them are never read and come back 0.  Returns a device array (B, T, n_mfcc)."""
        if len(rows.shape) != 3 or min(rows.shape) < 1:
            raise ValueError('mfcc: rows must be a non-empty (B, T, n_mels) array, got shape {}'.format(tuple(rows.shape)))
        B, T, n_mels = (int(d) for d in rows.shape)
        if int(n_mfcc) != n_mfcc or not 1 <= n_mfcc <= n_mels or n_mels > 1024:
            raise ValueError('mfcc: need 1 <= n_mfcc <= n_mels <= 1024, got n_mfcc = {!r}, n_mels = {}'.format(n_mfcc, n_mels))
        rows, stride = _strided_rows('mfcc', rows, B, T, n_mels, row_stride, 'n_mels')
        nf = stretch_frame_counts(n_frames, B, T)
        p_rows, _k = self._in(rows, np.float32)
        out = self.empty((B, T, int(n_mfcc)))
        self._check_or_free(self.lib.tts_mfcc(self.handle, p_rows, B, T, n_mels, stride, _int32_ptr(nf), int(n_mfcc), 1 if clip01 else 0,
                                              out.data_ptr()), out)
        return out

    def dtw_max_frames(self):
        """tts_dtw_max_frames: the longest sequence :meth:`dtw` takes."""
        return int(self.lib.tts_dtw_max_frames())

    def dtw_tile(self):
        """tts_dtw_tile: the cells of one piece of the kernel's cut of an anti-diagonal (no result depends on it)."""
        return int(self.lib.tts_dtw_tile())

    def dtw(self, a, b, n_a=None, n_b=None, D=None, want_path=False, skip=0):
        """tts_dtw: dynamic time warping of B pairs, ``a`` (B, Ta, K) against ``b`` (B, Tb, K), host arrays or device buffers,
        under the Euclidean distance of the frames -- floats ``skip`` .. ``skip + D - 1`` of every row (``D`` None: all behind
        ``skip``; ``skip`` = 1 leaves c0 out).  ``n_a`` / ``n_b``: B lengths (host integers); frames at or behind them are
        never read.  Returns the device arrays ``(cost, path_len)`` -- float64 (B,) and int32 (B,) -- and with ``want_path``
        also ``path`` int32 (B, Ta + Tb - 1, 2): rows k < path_len[b] are the (i, j) of the path from (0, 0), the rest
        (-1, -1).  include/sstts_hip.h has the definition: costs are the bits of tests/dtw_oracle.py."""
        if len(a.shape) != 3 or len(b.shape) != 3 or min(a.shape) < 1 or min(b.shape) < 1:
            raise ValueError('dtw: a and b must be non-empty (B, T, K) arrays, got shapes {} and {}'.format(tuple(a.shape), tuple(b.shape)))
        B, Ta, Ka = (int(d) for d in a.shape)
        Bb, Tb, Kb = (int(d) for d in b.shape)
        if Bb != B:
            raise ValueError('dtw: {} sequences in a and {} in b'.format(B, Bb))
        skip = int(skip)
        if skip < 0:
            raise ValueError('dtw: skip must be >= 0')
        D = min(Ka, Kb) - skip if D is None else D
        if int(D) != D or D < 1 or skip + D > min(Ka, Kb):
            raise ValueError('dtw: need 1 <= D and skip + D <= the row length, got D = {!r}, skip = {}, rows of {} and {}'.format(D, skip, Ka, Kb))
        na, nb = stretch_frame_counts(n_a, B, Ta), stretch_frame_counts(n_b, B, Tb)
        p_a, _ka = self._in(a, np.float32)
        p_b, _kb = self._in(b, np.float32)
        cost = self.empty((B,), np.float64)
        plen = self.empty((B,), np.int32)
        path = self.empty((B, Ta + Tb - 1, 2), np.int32) if want_path else None
        self._check_or_free(self.lib.tts_dtw(self.handle, p_a + 4 * skip, Ta, Ka, _int32_ptr(na), p_b + 4 * skip, Tb, Kb, _int32_ptr(nb), B, int(D),
                                             cost.data_ptr(), plen.data_ptr(), path.data_ptr() if want_path else None), cost, plen, path)
        return (cost, plen, path) if want_path else (cost, plen)

    # ------------------------------------------------------------------ F0 tracking
    def f0(self, wavs, sampling_rate, hop_length, fmin=60.0, fmax=500.0, window=1024, threshold=0.1, n_samples=None,
           want_aperiodicity=False, tau_min=None, tau_max=None):
        """tts_f0: the fundamental frequency of ``wavs`` -- one waveform (n,) or a batch (B, n), a host array or a device buffer --
        by YIN, one value per ``hop_length`` samples: frame t sits at sample t hop_length, 1 + n // hop_length frames.  The lags
        searched are tau_min = max(2, int(sr // fmax)) .. tau_max = ceil(sr / fmin) (or ``tau_min`` / ``tau_max`` as given), the
        sums run over ``window`` samples, a frame is voiced where the normalised difference falls below ``threshold``.
        ``n_samples``: B lengths (host integers) -- samples at or behind them are never read; None: all n.  Returns a device
        array (B, T) of Hz, 0 in unvoiced and padding frames and NaN where a frame's span holds a non-finite sample -- (T,) for
        a 1-D input -- and with ``want_aperiodicity`` also the normalised difference at the chosen lag, of the same shape.
        include/sstts_hip.h has the definition: the results are the bits of tests/f0_oracle.py."""
        wavs, single, B, n = _waveforms('f0', wavs)
        lo, hi = f0_lag_bounds(sampling_rate, fmin, fmax)
        lo = lo if tau_min is None else tau_min
        hi = hi if tau_max is None else tau_max
        if int(hop_length) != hop_length or hop_length < 1 or int(window) != window or int(lo) != lo or int(hi) != hi:
            raise ValueError('f0: hop_length >= 1, window and the lags must be integers, got {!r}, {!r}, {!r}, {!r}'.format(hop_length, window, lo, hi))
        if not 1 <= window <= F0_MAX_WINDOW:
            raise ValueError('f0: window = {} is not in 1 .. {} (tts_f0_max_window)'.format(window, F0_MAX_WINDOW))
        if not 2 <= lo <= hi <= F0_MAX_LAG:
            raise ValueError('f0: the lags {} .. {} are not 2 <= tau_min <= tau_max <= {} (tts_f0_max_lag): fmin is at least '
                             'sampling_rate / {}'.format(lo, hi, F0_MAX_LAG, F0_MAX_LAG))
        if np.isnan(float(threshold)):
            raise ValueError('f0: the threshold is NaN')
        ns = stretch_frame_counts(n_samples, B, n)
        p_wav, _k = self._in(wavs, np.float32)
        T = f0_frames(n, hop_length)
        out = self.empty((T,) if single else (B, T))
        ap = self.empty((T,) if single else (B, T)) if want_aperiodicity else None
        self._check_or_free(self.lib.tts_f0(self.handle, p_wav, B, n, _int32_ptr(ns), float(sampling_rate), int(hop_length), int(window), int(lo),
                                            int(hi), float(threshold), out.data_ptr(), ap.data_ptr() if ap is not None else None), out, ap)
        return (out, ap) if want_aperiodicity else out

    # ------------------------------------------------------------------ intelligibility
    def stoi(self, ref, deg, n_samples=None, extended=False, want_index=False, want_envelopes=False):
        """tts_stoi: short-time objective intelligibility (``extended``: ESTOI) of ``deg`` against the time-aligned ``ref`` -- one
        waveform (n,) each or batches (B, n) of one shape, host arrays or device buffers, AT 10 000 Hz (``audio.metrics.stoi``
        resamples).  ``n_samples``: B lengths (host integers) -- samples at or behind them are never read; None: all n.  Returns
        a host array (B,) of ``STOI_RECORD`` -- the frames, those kept (within 40 dB of the reference's loudest), the segments of
        30 kept frames, the terms that were 0 by rule, and the value: NaN with fewer than 30 kept frames or a NaN in a kept sample
        -- then, with ``want_index``, the kept frames' indices, int32 (B, cap) with cap = ``stoi_frames(n)`` (a row's first
        ``kept`` entries are written), and, with ``want_envelopes``, the band envelopes, float64 (B, 2, 15, cap): ref then deg (a
        row's first ``kept`` columns are written).  include/sstts_hip.h has the definition; tests/stoi_oracle.py restates it."""
        if isinstance(extended, (bool, np.bool_)):
            extended = int(extended)
        if isinstance(extended, float) or extended not in (0, 1):
            raise ValueError('stoi: extended must be False / True (0 / 1), got {!r}'.format(extended))
        ref, _single, B, n = _waveforms('stoi', ref)
        deg, _single_d, Bd, nd = _waveforms('stoi', deg)
        if (B, n) != (Bd, nd):
            raise ValueError('stoi: ref and deg must have one shape, got {} and {}'.format((B, n), (Bd, nd)))
        ns = _sample_lengths(n_samples, B, n)
        cap = stoi_frames(n)
        if cap > STOI_MAX_FRAMES:
            raise ValueError('stoi: {} frames are more than {} (tts_stoi_max_frames)'.format(cap, STOI_MAX_FRAMES))
        p_ref, keep_r = self._in(ref, np.float32)
        p_deg, keep_d = self._in(deg, np.float32)
        rec = self.empty((B, 3), np.float64)   # (B records of 24 bytes)
        index = self.empty((B, max(cap, 1)), np.int32) if want_index else None
        env = self.empty((B, 2, STOI_BANDS, max(cap, 1)), np.float64) if want_envelopes else None
        try:
            self._check_or_free(self.lib.tts_stoi(self.handle, p_ref, p_deg, B, n, _int32_ptr(ns), int(extended), rec.data_ptr(),
                                                  index.data_ptr() if want_index else None, env.data_ptr() if want_envelopes else None),
                                rec, index, env)
            answer = (_records(rec, STOI_RECORD),)
            for extra in (index, env):
                if extra is not None:
                    answer += (extra.to_host()[..., :cap],)
                    extra.free()
        finally:
            if keep_r is not ref:
                keep_r.free()
            if keep_d is not deg:
                keep_d.free()
        return answer if len(answer) > 1 else answer[0]

    def stoi_tables(self):
        """tts_stoi_window and tts_stoi_bands: the analysis window, float64 (256,), and the bands' bins [lo, hi), int32 (15, 2)."""
        w = np.zeros(256, np.float64)
        e = np.zeros((STOI_BANDS, 2), np.int32)
        self._check(self.lib.tts_stoi_window(w.ctypes.data_as(POINTER(ctypes.c_double))))
        self._check(self.lib.tts_stoi_bands(e.ctypes.data_as(POINTER(c_int32))))
        return w, e

    # ------------------------------------------------------------------ loudness
    def _ragged_waveforms(self, what, wavs, n_samples, lo=1):
        """``(wavs, single, B, n, the checked lengths or None)`` of a call on waveforms with per-utterance lengths in ``lo`` .. n"""
        wavs, single, B, n = _waveforms(what, wavs)
        return wavs, single, B, n, _sample_lengths(n_samples, B, n, lo)

    def _rows_out(self, what, wavs, single, out, B, n):
        """Where a stage that filters B rows of n samples puts them, ``(the input's pointer, the output array, whether that is
        fresh)``: ``out`` where one is given (a device buffer of the input's size, which may be the input), else a device input in
        place, a host input uploaded fresh -- a single waveform as (n,).  The stages that only work in place give ``out`` None."""
        if out is not None and (not _is_device(out) or int(np.prod(out.shape)) != B * n):
            raise ValueError('{}: out must be a device buffer of {} floats'.format(what, B * n))
        if out is None and not _is_device(wavs):
            out = self.to_device(np.ascontiguousarray(wavs, dtype=np.float32))
            if single:
                out.shape = (n,)
            return out.data_ptr(), out, True
        p_wav, _k = self._in(wavs, np.float32)
        return p_wav, wavs if out is None else out, False

    def _loudness_args(self, what, wavs, sampling_rate, n_samples):
        return (loudness_sampling_rate(what, sampling_rate),) + self._ragged_waveforms(what, wavs, n_samples)

    def loudness(self, wavs, sampling_rate, n_samples=None, return_mean_square=False, want_blocks=False):
        """tts_loudness: the integrated loudness after ITU-R BS.1770-4 / EBU R 128 of ``wavs`` -- one mono waveform (n,) or a
        batch (B, n), a host array or a device buffer -- in LUFS, a float64 host array (B,): -inf where no block passes the
        gates (silence, or less than 400 ms), NaN where a counted block holds a non-finite sample.  ``n_samples``: B lengths
        (host integers) -- samples at or behind them are never read; None: all n.  ``return_mean_square``: also the gated mean
        square z the figure is taken from (LUFS = -0.691 + 10 log10 z); ``want_blocks``: also int32 (B, 2), the blocks and
        those that passed both gates.  include/sstts_hip.h has the definition: z is the bits of tests/loudness_oracle.py."""
        sr, wavs, _single, B, n, ns = self._loudness_args('loudness', wavs, sampling_rate, n_samples)
        p_wav, _k = self._in(wavs, np.float32)
        z = self.empty((B,), np.float64)
        blocks = self.empty((B, 2), np.int32) if want_blocks else None
        self._check_or_free(self.lib.tts_loudness(self.handle, p_wav, B, n, _int32_ptr(ns), sr, z.data_ptr(),
                                                  blocks.data_ptr() if want_blocks else None), z, blocks)
        z_host = z.to_host()
        z.free()
        out = (lufs(z_host),) + ((z_host,) if return_mean_square else ())
        if want_blocks:
            out += (blocks.to_host(),)
            blocks.free()
        return out if len(out) > 1 else out[0]

    def loudness_normalize(self, wavs, sampling_rate, target_lufs=LOUDNESS_TARGET, max_peak=LOUDNESS_MAX_PEAK, n_samples=None,
                           return_mean_square=False):
        """tts_loudness_normalize: every utterance of ``wavs`` scaled to ``target_lufs`` by one gain, which no larger than
        ``max_peak`` / its peak.  Returns ``(waveforms, gains)``: a device array of the input's shape -- a device input is scaled
        in place and handed back, a host input is uploaded first -- and the float64 host array (B,) of the gains (1 where the
        utterance is silent, shorter than a block or holds a non-finite sample in one).  ``n_samples`` as in ``loudness``:
        samples at or behind them are neither read nor written.  ``return_mean_square``: also z as measured before the gain."""
        sr, wavs, single, B, n, ns = self._loudness_args('loudness_normalize', wavs, sampling_rate, n_samples)
        target, peak = loudness_target('loudness_normalize', target_lufs, max_peak)
        _p, out, fresh = self._rows_out('loudness_normalize', wavs, single, None, B, n)
        z, g = self.empty((B,), np.float64), self.empty((B,), np.float64)
        self._check_or_free(self.lib.tts_loudness_normalize(self.handle, out.data_ptr(), B, n, _int32_ptr(ns), sr, target, peak, z.data_ptr(),
                                                            g.data_ptr()), z, g, out if fresh else None)
        gains, z_host = g.to_host(), z.to_host()
        z.free()
        g.free()
        return (out, gains, z_host) if return_mean_square else (out, gains)

    # ------------------------------------------------------------------ true peak and limiter
    def true_peak(self, wavs, n_samples=None, want_sample_peak=False):
        """tts_true_peak: the peak of the 4x oversampled signal (ITU-R BS.1770-4 Annex 2) of ``wavs`` -- one mono waveform (n,)
        or a batch (B, n), a host array or a device buffer -- as a float64 host array (B,), linear (``dbtp`` makes dBTP of it);
        never below the sample peak, which ``want_sample_peak`` returns as well.  ``n_samples``: B lengths (host integers) --
        samples at or behind them are never read; None: all n.  The bits of tests/limiter_oracle.py."""
        wavs, _single, B, n, ns = self._ragged_waveforms('true_peak', wavs, n_samples)
        p_wav, _k = self._in(wavs, np.float32)
        tp = self.empty((B,), np.float64)
        sp = self.empty((B,), np.float64) if want_sample_peak else None
        self._check_or_free(self.lib.tts_true_peak(self.handle, p_wav, B, n, _int32_ptr(ns), tp.data_ptr(),
                                                   sp.data_ptr() if want_sample_peak else None), tp, sp)
        out = tp.to_host()
        tp.free()
        if want_sample_peak:
            out = (out, sp.to_host())
            sp.free()
        return out

    def limit(self, wavs, ceiling, lookahead=0, oversample=LIMIT_OVERSAMPLE, n_samples=None):
        """tts_limit: a look-ahead peak limiter over every utterance of ``wavs``: no finite sample of the result is above
        ``ceiling``, and a row that never was comes back as its own bits.  ``lookahead``: samples, 0 .. 1024; ``oversample``: 1
        (sample peaks) or 4 (the interpolated peaks ``true_peak`` reads).  Returns ``(waveforms, stats)``: a device array of the
        input's shape -- a device input is limited in place and handed back, a host input is uploaded first -- and a host array
        (B,) of ``LIMIT_RECORD``.  ``n_samples`` as in ``true_peak``: samples at or behind them are neither read nor written."""
        wavs, single, B, n, ns = self._ragged_waveforms('limit', wavs, n_samples)
        c, L, o = limit_arguments('limit', ceiling, lookahead, oversample)
        _p, out, fresh = self._rows_out('limit', wavs, single, None, B, n)
        st = self.empty((B, 2), np.float64)   # (B records of 16 bytes)
        self._check_or_free(self.lib.tts_limit(self.handle, out.data_ptr(), B, n, _int32_ptr(ns), c, L, o, st.data_ptr()), st, out if fresh else None)
        return out, _records(st, LIMIT_RECORD)

    # ------------------------------------------------------------------ the equaliser
    def equalize(self, wavs, sections, n_samples=None, out=None):
        """tts_equalize: every utterance of ``wavs`` -- one mono waveform (n,) or a batch (B, n), a host array or a device buffer --
        through a cascade of second-order sections.  ``sections``: an (S, 5) array of rows b0 b1 b2 a1 a2, S in 1 .. 8, or anything
        else ``equalizer_setting`` reads (a profile name, ``(kind, f0_hz, q, gain_db)`` sections: designed at the model's sampling
        rate).  Returns a device array of the input's shape: ``out`` where one is given (a device buffer of the input's size, which
        may be the input), else a device input filtered in place and handed back, a host input uploaded first.  ``n_samples``: B
        lengths (host integers) -- samples at or behind them are neither read nor written; None: all n.  The bits of
        tests/equalizer_oracle.py."""
        wavs, single, B, n, ns = self._ragged_waveforms('equalize', wavs, n_samples)
        setting = equalizer_setting(sections)
        if setting is None:
            raise ValueError('equalize: sections are needed')
        sos = equalizer_sections(setting, self.sampling_rate)
        p_wav, out, fresh = self._rows_out('equalize', wavs, single, out, B, n)
        self._check_or_free(self.lib.tts_equalize(self.handle, p_wav, out.data_ptr(), B, n, _int32_ptr(ns),
                                                  sos.ctypes.data_as(POINTER(ctypes.c_double)), len(sos)), out if fresh else None)
        return out

    # ------------------------------------------------------------------ the compressor
    def compress(self, wavs, params, n_samples=None, out=None, envelope=False, stats=False):
        """tts_compress: a feed-forward peak compressor over every utterance of ``wavs`` -- one mono waveform (n,) or a batch (B, n),
        a host array or a device buffer.  ``params``: what ``compressor_setting`` reads -- a profile name, ``(threshold_db, ratio,
        knee_db, attack_ms, release_ms, makeup_db)`` (coefficients made at the model's sampling rate) or ``('params', (threshold_db,
        slope, knee_db, makeup_db, attack_coeff, release_coeff))``.  Returns a device array of the input's shape: ``out`` where one
        is given (a device buffer of the input's size, which may be the input), else a device input compressed in place and handed
        back, a host input uploaded first.  ``n_samples``: B lengths (host integers) -- samples at or behind them are neither read
        nor written; None: all n.  ``envelope``: also a float64 device array (B, n), the detector's e of every sample (what lies at
        or behind a row's length is not written); ``stats``: also a host array (B,) of ``COMPRESS_RECORD``.  The envelope is the
        bits of tests/compressor_oracle.py."""
        wavs, single, B, n, ns = self._ragged_waveforms('compress', wavs, n_samples)
        setting = compressor_setting(params)
        if setting is None:
            raise ValueError('compress: parameters are needed')
        p = TtsCompressor(*compressor_params(setting, self.sampling_rate))
        p_wav, out, fresh = self._rows_out('compress', wavs, single, out, B, n)
        env = self.empty((B, n), np.float64) if envelope else None
        st = self.empty((B, 2), np.float64) if stats else None   # (B records of 16 bytes)
        self._check_or_free(self.lib.tts_compress(self.handle, p_wav, out.data_ptr(), B, n, _int32_ptr(ns), ctypes.addressof(p),
                                                  env.data_ptr() if envelope else None, st.data_ptr() if stats else None),
                            out if fresh else None, env, st)
        answer = (out,) + ((env,) if envelope else ()) + ((_records(st, COMPRESS_RECORD),) if stats else ())
        return answer if len(answer) > 1 else out

    # ------------------------------------------------------------------ the watermark
    def _watermark_args(self, what, wavs, watermark, n_samples):
        wavs, single, B, n = _waveforms(what, wavs)
        setting = watermark_setting(watermark)
        if setting is None:
            raise ValueError('{}: a key is needed'.format(what))
        return wavs, single, B, n, _sample_lengths(n_samples, B, n, 0), TtsWatermark(*setting)

    def watermark_embed(self, wavs, watermark, n_samples=None, out=None, stats=False):
        """tts_watermark_embed: a keyed spread-spectrum carrier under the local envelope added to every utterance of ``wavs`` -- one
        mono waveform (n,) or a batch (B, n), a host array or a device buffer.  ``watermark``: what ``watermark_setting`` reads -- a
        key, ``(key, payload)`` or ``(key, payload, payload_bits, chip, chips_per_symbol, strength)``; the defaults are UNTUNED.
        Returns a device array of the input's shape: ``out`` where one is given (a device buffer of the input's size, which may be
        the input), else a device input marked in place and handed back, a host input uploaded first.  ``n_samples``: B lengths in
        0 .. n (host integers) -- samples at or behind them carry no mark; None: all n.  ``stats``: also a host array (B,) of
        ``WATERMARK_EMBED_RECORD``.  The bits of tests/watermark_oracle.py."""
        wavs, single, B, n, ns, p = self._watermark_args('watermark_embed', wavs, watermark, n_samples)
        p_wav, out, fresh = self._rows_out('watermark_embed', wavs, single, out, B, n)
        st = self.empty((B, 2), np.float64) if stats else None   # (B records of 16 bytes)
        self._check_or_free(self.lib.tts_watermark_embed(self.handle, p_wav, out.data_ptr(), B, n, _int32_ptr(ns), ctypes.addressof(p),
                                                         st.data_ptr() if stats else None), out if fresh else None, st)
        return (out, _records(st, WATERMARK_EMBED_RECORD)) if stats else out

    def watermark_detect(self, wavs, watermark, offsets=64, n_samples=None, want_scores=False, want_sums=False):
        """tts_watermark_detect: the search for the carrier of ``watermark`` (its key and its shape; the payload and the strength are
        not read) in every utterance of ``wavs`` -- one mono waveform (n,) or a batch (B, n), a host array or a device buffer -- over
        the offsets 0 .. ``offsets`` - 1 (1 .. 4096): how many samples the row may have lost at its front.  Returns a host array
        (B,) of ``WATERMARK_DETECT_RECORD`` -- the lowest offset with the largest score, the score, the energy there and the payload
        read; ``watermark_zeta`` makes the statistic of them -- then, with ``want_scores``, every offset's score, int64 (B, offsets),
        and, with ``want_sums``, the payload bits' sums at the offset found, int64 (B, payload_bits).  ``n_samples``: B lengths in
        0 .. n; None: all n.  The bits of tests/watermark_oracle.py."""
        wavs, _single, B, n, ns, p = self._watermark_args('watermark_detect', wavs, watermark, n_samples)
        D = offsets
        if isinstance(D, (bool, np.bool_)) or not isinstance(D, (int, np.integer)) or not 1 <= D <= WM_MAX_OFFSETS:
            raise ValueError('watermark_detect: offsets must be an integer in 1 .. {}, got {!r}'.format(WM_MAX_OFFSETS, D))
        p_wav, keep = self._in(wavs, np.float32)
        rec = self.empty((B, 4), np.float64)   # (B records of 32 bytes)
        scores = self.empty((B, int(D)), np.int64) if want_scores else None
        sums = self.empty((B, p.payload_bits), np.int64) if want_sums else None
        self._check_or_free(self.lib.tts_watermark_detect(self.handle, p_wav, B, n, _int32_ptr(ns), ctypes.addressof(p), int(D), rec.data_ptr(),
                                                          scores.data_ptr() if want_scores else None, sums.data_ptr() if want_sums else None),
                            rec, scores, sums)
        answer = (_records(rec, WATERMARK_DETECT_RECORD),)
        for extra in (scores, sums):
            if extra is not None:
                answer += (extra.to_host(),)
                extra.free()
        if keep is not wavs:
            keep.free()
        return answer if len(answer) > 1 else answer[0]

    # ------------------------------------------------------------------ delivery formats
    def encode(self, wav, format, dither='tpdf', seed=0, n_samples=None):
        """tts_encode: float32 rows to delivery codes -- ``format`` 'pcm16' (int16), 'pcm8', 'mulaw' or 'alaw' (uint8) -- in one
        pass on the device: scaled, dithered (``dither`` 'tpdf' or None; a function of ``seed``, the row and the sample index
        alone), rounded to the nearest with ties to even, saturated.  ``wav``: one waveform (n,) or a batch (B, n), a host array
        or a device buffer.  ``n_samples``: B lengths in 0 .. n (host integers) -- samples at or behind them are not read and come
        out as the format's silence; None: all n.  Returns ``(codes, stats)``: the codes in the input's shape -- a device array for
        a device input, a host array for a host input -- and a host array (B,) of ``ENCODE_RECORD``.  The bits of
        tests/encode_oracle.py."""
        f = format_value('encode', format, encoding=True)
        d = dither_value('encode', dither)
        if isinstance(seed, (bool, np.bool_)) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError('encode: the seed must be an integer in 0 .. 2^64 - 1, got {!r}'.format(seed))
        wav, single, B, n, ns = self._ragged_waveforms('encode', wav, n_samples, 0)
        on_device = _is_device(wav)
        p_wav, _k = self._in(wav, np.float32)
        out = self.empty((n,) if single else (B, n), FORMAT_DTYPES[f])
        st = self.empty((B, 4), np.int32)   # (B records of 16 bytes)
        self._check_or_free(self.lib.tts_encode(self.handle, p_wav, B, n, _int32_ptr(ns), f, d, int(seed), out.data_ptr(), st.data_ptr()), out, st)
        stats = _records(st, ENCODE_RECORD)
        if not on_device:
            codes = out.to_host()
            out.free()
            return codes, stats
        return out, stats

    # ------------------------------------------------------------------ attention diagnostics
    def alignment_stats(self, alignments, n_sent=None, n_steps=None, want_durations=False, want_pos=False):
        """tts_alignment_stats: what an alignment history says about whether the sentence was read.  ``alignments``
        (n_steps_max, B, Ts) float32 as the decoder writes them, a host array or a device buffer; ``n_sent``: B sentence lengths
        (host integers, None: all Ts) -- columns at or behind them count as padding; ``n_steps``: B step counts (None: all
        n_steps_max) -- steps at or behind them are never read.  Returns a host array (B,) of ``ALIGNMENT_RECORD`` -- n_sent,
        n_steps, reached, end_step, backward, max_back, max_jump, longest_stall, after_end, off_text, skipped, reserved and
        focus_sum (mean focus = focus_sum / n_steps) -- then, with ``want_durations``, the int32 host array (B, Ts) of the
        steps spent on every token, and with ``want_pos`` the positions int32 (B, n_steps_max) (-1 behind an utterance's steps)
        and their weights float32 (B, n_steps_max) (0 there).  include/sstts_hip.h has the definition: the records are the bits
        of tests/alignment_oracle.py.  ``tacotron.attention_check.verdict`` turns them into flags."""
        shape = tuple(int(d) for d in alignments.shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('alignment_stats: alignments (n_steps_max, B, Ts) are needed, got shape {}'.format(shape))
        S, B, Ts = shape
        ns = alignment_lengths(n_sent, B, Ts, 'n_sent', 'Ts')
        nt = alignment_lengths(n_steps, B, S, 'n_steps', 'n_steps_max')
        p_ali, _k = self._in(alignments, np.float32)
        stats = self.empty((B,), ALIGNMENT_RECORD)
        dur = self.empty((B, Ts), np.int32) if want_durations else None
        pos = self.empty((B, S), np.int32) if want_pos else None
        peak = self.empty((B, S), np.float32) if want_pos else None
        self._check_or_free(self.lib.tts_alignment_stats(self.handle, p_ali, S, B, Ts, _int32_ptr(ns), _int32_ptr(nt), stats.data_ptr(),
                                                         dur.data_ptr() if dur is not None else None,
                                                         pos.data_ptr() if pos is not None else None,
                                                         peak.data_ptr() if peak is not None else None), stats, dur, pos, peak)
        out = ()
        for a in (stats, dur, pos, peak):
            if a is not None:
                out += (a.to_host(),)
                a.free()
        return out if len(out) > 1 else out[0]

    def set_token_times(self, enabled, pad_id=0, max_jump=4):
        """tts_set_token_times: the handle's setting, read by every synthesize / synthesize_host call made after it.  On, every
        call also searches its alignments for the best monotone path (``token_times``), the sentence lengths taken from its ids
        with ``pad_id`` as the padding: ``synth_token_times`` / ``wait_host_token_times`` fetch the results."""
        setting = token_times_setting((bool(enabled), pad_id, max_jump))
        self._check(self.lib.tts_set_token_times(self.handle, 1 if setting[0] else 0, setting[1], setting[2]))
        self._token_times = setting

    def synth_token_times(self, B):
        """tts_synth_token_times: ``(start, stats)`` -- int32 (B, Ts + 1) and (B,) of ``TOKEN_TIMES_RECORD``, host arrays -- of the
        last ``synthesize`` / ``synthesize_host`` call made on the handle with the timing marks on.  Waits for that call's
        decoder, not for its Griffin-Lim."""
        Ts = getattr(self, '_token_times_Ts', None)
        if Ts is None:
            raise ValueError('synth_token_times: no synthesize call has been made with token_times on')
        start = np.zeros((int(B), Ts + 1), dtype=np.int32)
        stats = np.zeros(int(B), dtype=TOKEN_TIMES_RECORD)
        self._check(self.lib.tts_synth_token_times(self.handle, start.ctypes.data, stats.ctypes.data, int(B)))
        return start, stats

    def wait_host_token_times(self, ticket):
        """``(start, stats)`` (copies) of a ``synthesize_host`` call made with the timing marks on: tts_wait_host_token_times.
        Waits like ``wait_host`` and does not consume the ticket."""
        ps, pr = c_void_p(), c_void_p()
        n, ts = c_int(0), c_int(0)
        self._check(self.lib.tts_wait_host_token_times(self.handle, int(ticket), byref(ps), byref(pr), byref(n), byref(ts)))
        start = np.frombuffer(ctypes.string_at(ps.value, n.value * (ts.value + 1) * 4), dtype=np.int32).reshape(n.value, ts.value + 1).copy()
        stats = np.frombuffer(ctypes.string_at(pr.value, n.value * TOKEN_TIMES_RECORD.itemsize), dtype=TOKEN_TIMES_RECORD).copy()
        return start, stats

    def text_lengths(self, ids, pad_id=0):
        """tts_text_lengths: the sentence lengths of padded ids (B, Ts) int32, host or device -- 1 + the last position that does
        not hold ``pad_id``, 1 for a row of padding -- as an int32 host array (B,)."""
        shape = tuple(int(d) for d in ids.shape)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError('text_lengths: ids (B, Ts) are needed, got shape {}'.format(shape))
        if not isinstance(pad_id, (int, np.integer)) or isinstance(pad_id, bool) or not -2 ** 31 <= int(pad_id) < 2 ** 31:
            raise ValueError('text_lengths: pad_id must be an int32, got {!r}'.format(pad_id))
        p_ids, _k = self._in(ids, np.int32)
        out = self.empty((shape[0],), np.int32)
        self._check_or_free(self.lib.tts_text_lengths(self.handle, p_ids, shape[0], shape[1], int(pad_id), out.data_ptr()), out)
        n = out.to_host()
        out.free()
        return n

    def token_times(self, alignments, n_sent=None, n_steps=None, max_jump=4, want_path=False, to_host=True):
        """tts_token_times: when every token is spoken -- the best monotone path through an alignment history, a position per
        step that never goes back and advances by at most ``max_jump`` (1 .. 15) tokens a step.  ``alignments`` (n_steps_max, B,
        Ts) float32 as the decoder writes them, a host array or a device buffer; ``n_sent`` / ``n_steps`` as ``alignment_stats``
        takes them -- columns and steps at or behind them are never read.  Returns ``start``, the int32 host array (B, Ts + 1) --
        token j of utterance b is spoken during the decoder steps ``start[b, j] .. start[b, j + 1]`` -- and a host array (B,) of
        ``TOKEN_TIMES_RECORD`` -- score, n_sent, n_steps, last, jumps, skipped, agree --, then with ``want_path`` the path int32
        (B, n_steps_max) (-1 behind an utterance's steps).  ``max_jump = 4`` is untuned: four characters per step of r frames.
        include/sstts_hip.h has the definition: everything is the bits of tests/marks_oracle.py.  ``tacotron.marks`` turns
        ``start`` into times.  ``to_host`` False: the device arrays as they are, nothing downloaded and nothing waited for (the
        caller downloads and frees them)."""
        shape = tuple(int(d) for d in alignments.shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('token_times: alignments (n_steps_max, B, Ts) are needed, got shape {}'.format(shape))
        S, B, Ts = shape
        ns = alignment_lengths(n_sent, B, Ts, 'n_sent', 'Ts')
        nt = alignment_lengths(n_steps, B, S, 'n_steps', 'n_steps_max')
        J = token_times_jump(max_jump)
        if Ts > TOKEN_TIMES_MAX_TOKENS:
            raise ValueError('token_times: Ts = {} is above the {} tokens of a table'.format(Ts, TOKEN_TIMES_MAX_TOKENS))
        p_ali, _k = self._in(alignments, np.float32)
        start = self.empty((B, Ts + 1), np.int32)
        stats = self.empty((B,), TOKEN_TIMES_RECORD)
        path = self.empty((B, S), np.int32) if want_path else None
        self._check_or_free(self.lib.tts_token_times(self.handle, p_ali, S, B, Ts, _int32_ptr(ns), _int32_ptr(nt), J, start.data_ptr(),
                                                     path.data_ptr() if path is not None else None, stats.data_ptr()), start, stats, path)
        if not to_host:
            return tuple(a for a in (start, stats, path) if a is not None)
        out = ()
        for a in (start, stats, path):
            if a is not None:
                out += (a.to_host(),)
                a.free()
        return out

    def synth_alignment_stats(self, B):
        """tts_synth_alignment_stats: the B records (``ALIGNMENT_RECORD``, a host array) of the last ``synthesize`` /
        ``synthesize_host`` call made on the handle with the attention diagnostics on.  Waits for that call's decoder, not for
        its Griffin-Lim."""
        out = np.zeros(int(B), dtype=ALIGNMENT_RECORD)
        self._check(self.lib.tts_synth_alignment_stats(self.handle, out.ctypes.data, int(B)))
        return out

    def wait_host_alignment_stats(self, ticket):
        """The B records (``ALIGNMENT_RECORD``, a copy) of a ``synthesize_host`` call made with the attention diagnostics on:
        tts_wait_host_alignment_stats.  Waits like ``wait_host`` and does not consume the ticket."""
        p = c_void_p()
        n = c_int(0)
        self._check(self.lib.tts_wait_host_alignment_stats(self.handle, int(ticket), byref(p), byref(n)))
        raw = ctypes.string_at(p.value, n.value * ALIGNMENT_RECORD.itemsize)
        return np.frombuffer(raw, dtype=ALIGNMENT_RECORD).copy()

    def f0_compare(self, f0_a, f0_b, path):
        """tts_f0_compare: the F0 and voicing errors of B pairs of tracks, ``f0_a`` (B, Ta) against ``f0_b`` (B, Tb) -- side b is
        the recording -- along ``path`` (B, rows, 2) int32 as :meth:`dtw` writes it (rows with a negative entry are skipped); host
        arrays or device buffers.  Returns the device arrays ``(counts, sums)``: int32 (B, 5) = steps, both voiced, one side
        voiced, gross pitch errors (beyond 20 %), NaN steps; float64 (B, 2) = the sums of (fa - fb) ** 2 in Hz ** 2 and of
        (1200 log2(fa / fb)) ** 2 in cents ** 2 over the steps voiced on both sides."""
        if len(f0_a.shape) != 2 or len(f0_b.shape) != 2 or len(path.shape) != 3 or min(f0_a.shape) < 1 or min(f0_b.shape) < 1 or \
                min(path.shape) < 1 or path.shape[2] != 2:
            raise ValueError('f0_compare: (B, Ta) and (B, Tb) tracks and a (B, rows, 2) path are needed, got shapes {}, {} and {}'.format(
                tuple(f0_a.shape), tuple(f0_b.shape), tuple(path.shape)))
        B, Ta = (int(d) for d in f0_a.shape)
        Bb, Tb = (int(d) for d in f0_b.shape)
        rows = int(path.shape[1])
        if Bb != B or int(path.shape[0]) != B:
            raise ValueError('f0_compare: {} tracks in f0_a, {} in f0_b and {} paths'.format(B, Bb, path.shape[0]))
        p_a, _ka = self._in(f0_a, np.float32)
        p_b, _kb = self._in(f0_b, np.float32)
        p_p, _kp = self._in(path, np.int32)
        counts = self.empty((B, 5), np.int32)
        sums = self.empty((B, 2), np.float64)
        self._check_or_free(self.lib.tts_f0_compare(self.handle, p_a, Ta, p_b, Tb, p_p, rows, B, counts.data_ptr(), sums.data_ptr()), counts, sums)
        return counts, sums

    # ------------------------------------------------------------------ speaking rate
    def stretched_frames(self, n, rate):
        """tts_stretched_frames: the frames of a time-stretched utterance of ``n`` frames, ceil(n / rate)."""
        r = speaking_rate_value(rate)
        if r is None or int(n) != n or n < 1:
            raise ValueError('stretched_frames: need n >= 1 frames and a rate, got {!r}, {!r}'.format(n, rate))
        out = c_int(0)
        rc = self.lib.tts_stretched_frames(int(n), r, byref(out))
        if rc != TTS_OK:
            raise ValueError('stretched_frames({!r}, {!r}) refused'.format(n, rate))
        return out.value

    def _stretch_args(self, what, shape, T, rate, n_frames, T_out):
        r = speaking_rate_value(rate)
        if r is None:
            raise ValueError('{}: a rate in [0.25, 4] is needed'.format(what))
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('{}: a non-empty 3-D array is needed, got shape {}'.format(what, tuple(shape)))
        B = int(shape[0])
        nf = stretch_frame_counts(n_frames, B, T)
        longest = max(stretched_frames(n, r) for n in (nf.tolist() if nf is not None else [T]))
        T_out = longest if T_out is None else int(T_out)
        if T_out < longest:
            raise ValueError('{}: T_out = {} is smaller than the longest stretched utterance, {} frames'.format(what, T_out, longest))
        return r, nf, T_out

    def stretch_magnitudes(self, mag, rate, n_frames=None, T_out=None):
        """tts_stretch_magnitudes: the reference's time_stretch as far as it reaches Griffin-Lim (audio/effects.py:46-88) on
        ``mag`` (B, F, T), the layout of ``griffin_lim`` and ``stft_magnitude`` -- a host array or a device buffer.  Frame k
        of the result is the blend (1 - a) mag[:, :, i] + a mag[:, :, i + 1] at s = k rate, i = int(s), a = s - i, in double,
        rounded once.  ``n_frames``: B lengths (host integers) -- columns at or behind them are never read; None: all T.
        Returns a device array (B, F, T_out): utterance b holds ceil(n_frames[b] / rate) frames and zeros behind them;
        ``T_out`` None: the longest stretched length."""
        r, nf, T_out = self._stretch_args('stretch_magnitudes', mag.shape, int(mag.shape[2]) if len(mag.shape) == 3 else 0,
                                          rate, n_frames, T_out)
        B, F, T = (int(d) for d in mag.shape)
        p_mag, _k = self._in(mag, np.float32)
        out = self.empty((B, F, T_out))
        self._check_or_free(self.lib.tts_stretch_magnitudes(self.handle, p_mag, B, F, T, _int32_ptr(nf), r, T_out, out.data_ptr()), out)
        return out

    def stretch_rows(self, spec, rate, n_frames=None, T_out=None, row_stride=None):
        """tts_stretch_rows: the same blend on time-major rows, ``spec`` (B, T, F) as ``speech_frames`` takes it (``row_stride``
        as there: a device buffer of B * T * row_stride floats, or the view ``a[:, :, :F]`` of a contiguous host array; any
        other host array is uploaded with NaN in the padding columns).  Returns a device array (B, T_out, row_stride) of which
        the first F columns are written."""
        r, nf, T_out = self._stretch_args('stretch_rows', spec.shape, int(spec.shape[1]) if len(spec.shape) == 3 else 0,
                                          rate, n_frames, T_out)
        B, T, F = (int(d) for d in spec.shape)
        spec, stride = _strided_rows('stretch_rows', spec, B, T, F, row_stride)
        p_spec, _k = self._in(spec, np.float32)
        out = self.empty((B, T_out, stride))
        self._check_or_free(self.lib.tts_stretch_rows(self.handle, p_spec, B, T, F, stride, _int32_ptr(nf), r, T_out, out.data_ptr()), out)
        return out

    # ------------------------------------------------------------------ prosody: the segment-wise warp
    def warp_max_segments(self):
        """tts_warp_max_segments: the most segments :meth:`warp_magnitudes` takes in one call."""
        return int(self.lib.tts_warp_max_segments())

    def warp_tile(self):
        """tts_warp_tile: the output frames of a segment one workgroup of the warp writes."""
        return int(self.lib.tts_warp_tile())

    def warp_plan(self, shape, segments, n_frames=None):
        """tts_warp_plan, host only: the lengths ``n_out`` (int64 (B,)) of the rows that ``segments`` -- a WARP_SEGMENT array or rows
        ``(row, first, frames, pause, step, gain)`` -- make of a batch of ``shape`` (B, F, T) whose rows hold ``n_frames`` frames
        (None: all T).  ValueError for a list tts_warp_magnitudes refuses (``warp_list``), raised before the library is reached."""
        if len(shape) != 3:
            raise ValueError('warp_plan: the shape of a batch (B, F, T) is needed, got {!r}'.format(tuple(shape)))
        B, T = int(shape[0]), int(shape[2])
        q, nf, n_out, _count = warp_list(segments, B, T, n_frames)
        out = np.zeros(B, dtype=np.int64)
        rc = self.lib.tts_warp_plan(q.ctypes.data, q.shape[0], B, T, _int32_ptr(nf), out.ctypes.data_as(POINTER(c_int64)))
        self._host_plan_check(rc)
        assert (out == n_out).all(), (out, n_out)
        return out

    def warp_magnitudes(self, mag, segments, n_frames=None, T_out=None):
        """tts_warp_magnitudes: ``stretch_magnitudes`` with a rate, a gain and pauses that vary along the utterance, on ``mag``
        (B, F, T) -- a host array, which is uploaded, or a device buffer, which is read in place.  ``segments``: a WARP_SEGMENT
        array or rows ``(row, first, frames, pause, step, gain)``, the segments of a row one behind the other and the rows in
        order: source frames [first, first + frames) of the row at ``step`` / 65536 source frames per output frame, scaled by
        ``gain``, or (frames == 0) ``pause`` output frames of silence.  ``n_frames``: B lengths (host integers) -- frames at or
        behind them are never read; None: all T.  include/sstts_hip.h has the definition: the bits of tests/warp_oracle.py.

        Returns ``(out, n_out)``: a fresh device array (B, F, T_out) and the int64 host lengths (B,) -- row b holds n_out[b] frames
        followed by +0.0.  ``T_out`` None: the largest length.  ValueError for what the library refuses, raised before it is
        reached."""
        if len(mag.shape) != 3 or min(mag.shape) < 1:
            raise ValueError('warp_magnitudes: a non-empty 3-D array is needed, got shape {}'.format(tuple(mag.shape)))
        B, F, T = (int(d) for d in mag.shape)
        q, nf, n_out, _count = warp_list(segments, B, T, n_frames)
        longest = int(n_out.max())
        if T_out is None:
            T_out = longest
        if int(T_out) != T_out or not longest <= T_out <= WARP_MAX_T_OUT:
            raise ValueError('warp_magnitudes: T_out = {!r} is not in n_out.max() = {} .. 2^30'.format(T_out, longest))
        p_mag, _k = self._in(mag, np.float32)
        out = self.empty((B, F, int(T_out)))
        self._check_or_free(self.lib.tts_warp_magnitudes(self.handle, p_mag, B, F, T, _int32_ptr(nf), q.ctypes.data, q.shape[0], int(T_out),
                                                         out.data_ptr()), out)
        return out, n_out

    # ------------------------------------------------------------------ formant-preserving pitch: the envelope shift
    def shift_max_segments(self):
        """tts_shift_max_segments: the most segments :meth:`shift_magnitudes` takes in one call."""
        return int(self.lib.tts_shift_max_segments())

    def shift_tile(self):
        """tts_shift_tile: the frames of a computed segment one workgroup of the shift takes."""
        return int(self.lib.tts_shift_tile())

    def shift_max_order(self):
        """tts_shift_max_order: the largest order of the envelope."""
        return int(self.lib.tts_shift_max_order())

    def shift_plan(self, shape, segments, n_frames=None, order=None):
        """tts_shift_plan, host only: the library's checks of ``segments`` -- a SHIFT_SEGMENT array or rows ``(row, first, frames,
        pitch_step, formant_step)`` -- on a batch of ``shape`` (B, F, T) whose rows hold ``n_frames`` frames (None: all T) at
        ``order`` (None: ``shift_order`` of the model's sampling rate).  Returns the launches the call would make.  ValueError for a
        list tts_shift_magnitudes refuses (``shift_list``), raised before the library is reached."""
        if len(shape) != 3:
            raise ValueError('shift_plan: the shape of a batch (B, F, T) is needed, got {!r}'.format(tuple(shape)))
        B, F, T = (int(d) for d in shape)
        order = shift_order(self.sampling_rate) if order is None else order
        q, nf = shift_list(segments, B, F, T, n_frames, order)
        rc = self.lib.tts_shift_plan(q.ctypes.data, q.shape[0], B, F, T, _int32_ptr(nf), int(order))
        self._host_plan_check(rc)
        return shift_launches(q.shape[0])

    def shift_magnitudes(self, mag, segments, n_frames=None, order=None, out=None):
        """tts_shift_magnitudes: a pitch change that leaves the formants where they are, on ``mag`` (B, F, T) -- a host array, which is
        uploaded, or a device buffer, which is read in place; F = N + 1 with N a power of two, 128 .. 2048.  ``segments``: a
        SHIFT_SEGMENT array or rows ``(row, first, frames, pitch_step, formant_step)``, the segments of a row ascending and
        the rows in order: in the frames [first, first + frames) the fine structure (the harmonics) is read at ``pitch_step`` /
        65536 and the cepstral envelope of ``order`` coefficients at ``formant_step`` / 65536 source bins per output bin
        (``shift_step(semitones)`` makes a step).  Frames no segment covers, and segments at 65536 / 65536, are copied bit for bit;
        frames at or behind ``n_frames`` (B host integers; None: all T) are never read and come out +0.0.  ``order`` None:
        ``shift_order`` of the model's sampling rate (33 at 22 050 Hz).  include/sstts_hip.h has the definition.

        Returns a device array (B, F, T): ``out`` where one is given (a device buffer of that shape, not ``mag``), else a fresh one.
        ValueError for what the library refuses, raised before it is reached."""
        if len(mag.shape) != 3 or min(mag.shape) < 1:
            raise ValueError('shift_magnitudes: a non-empty 3-D array is needed, got shape {}'.format(tuple(mag.shape)))
        B, F, T = (int(d) for d in mag.shape)
        order = shift_order(self.sampling_rate) if order is None else order
        q, nf = shift_list(segments, B, F, T, n_frames, order)
        p_mag, _k = self._in(mag, np.float32)
        if out is not None:
            if tuple(out.shape) != (B, F, T) or not hasattr(out, 'data_ptr'):
                raise ValueError('shift_magnitudes: out must be a device buffer of shape {}'.format((B, F, T)))
            self._check(self.lib.tts_shift_magnitudes(self.handle, p_mag, B, F, T, _int32_ptr(nf), q.ctypes.data, q.shape[0], int(order),
                                                      out.data_ptr()))
            return out
        res = self.empty((B, F, T))
        self._check_or_free(self.lib.tts_shift_magnitudes(self.handle, p_mag, B, F, T, _int32_ptr(nf), q.ctypes.data, q.shape[0], int(order),
                                                          res.data_ptr()), res)
        return res

    def time_stretch(self, wavs, rate, n_iter=25, seed=0, want_magnitudes=False):
        """The reference's waveform effect time_stretch (audio/effects.py:46-88) as a composition of existing calls:
        ``stft_magnitude`` (n_fft 1024, window 1024, hop 256, power 1), ``stretch_magnitudes``, then ``griffin_lim`` in the
        general kernels from phases drawn from ``seed`` (the reference draws np.random.rand).  ``wavs``: one waveform (n,) or
        a uniform batch (B, n), host or device.  Returns a device array (B, 256 (T' - 1)) -- (256 (T' - 1),) for one waveform
        given as a 1-D host array -- with T' = ceil((1 + n // 256) / rate); with ``want_magnitudes`` also the device arrays
        (|STFT|, stretched) that were fed through."""
        r = speaking_rate_value(rate)
        if r is None:
            raise ValueError('time_stretch: a rate in [0.25, 4] is needed')
        wavs, single, _B, n = _waveforms('time_stretch', wavs, uniform=True)
        n_fft, win, hop = 1024, 1024, 256
        T = 1 + n // hop
        if hop * (stretched_frames(T, r) - 1) <= n_fft // 2:
            raise ValueError('time_stretch: {} samples at rate {} leave a signal shorter than n_fft / 2'.format(n, r))
        mag = self.stft_magnitude(wavs, n_fft, win, hop, 1.0)
        st = self.stretch_magnitudes(mag, r)
        wav, _mse = self.griffin_lim(st, int(n_iter), win, hop, n_fft, seed=seed, want_mse=False)
        if single:
            wav.shape = (wav.shape[1],)
        return (wav, mag, st) if want_magnitudes else wav

    # ------------------------------------------------------------------ resampling and pitch
    def resampled_length(self, n, ratio):
        """tts_resampled_length: ceil(n * ratio), the samples librosa.core.resample returns for ``n``."""
        r = resample_ratio_value(ratio)
        if int(n) != n or n < 1:
            raise ValueError('resampled_length: need n >= 1 samples, got {!r}'.format(n))
        out = c_int(0)
        if self.lib.tts_resampled_length(int(n), r, byref(out)) != TTS_OK:
            raise ValueError('resampled_length({!r}, {!r}) refused'.format(n, ratio))
        return out.value

    def resample(self, wavs, ratio, n_samples=None, N_out=None):
        """tts_resample: librosa 0.6 ``resample(..., res_type='kaiser_best')`` (resampy's windowed sinc) by ``ratio`` = target
        rate / source rate in [0.25, 4].  ``wavs``: one waveform (n,) or a batch (B, n), a host array or a device buffer.
        ``n_samples``: B lengths (host integers) -- samples at or behind them are never read; None: all n.  Returns a device
        array (B, N_out) -- (N_out,) for one waveform given as a 1-D array, host or device: utterance b holds min(int(n_samples[b] * ratio),
        N_out) resampled samples and zeros behind them; ``N_out`` None: ceil(longest * ratio), librosa's length."""
        r = resample_ratio_value(ratio)
        wavs, single, B, n = _waveforms('resample', wavs)
        ns = _sample_lengths(n_samples, B, n)
        if N_out is None:
            N_out = resampled_length(int(ns.max()) if ns is not None else n, r)
        N_out = int(N_out)
        if N_out < 1:
            raise ValueError('resample: N_out = {} < 1'.format(N_out))
        p_wav, _k = self._in(wavs, np.float32)
        out = self.empty((B, N_out))
        self._check_or_free(self.lib.tts_resample(self.handle, p_wav, B, n, _int32_ptr(ns), r, N_out, out.data_ptr()), out)
        if single:
            out.shape = (N_out,)
        return out

    def resample_segments_max(self):
        """tts_resample_segments_max: the most segments :meth:`resample_segments` takes in one call."""
        return int(self.lib.tts_resample_segments_max())

    def resample_segments_max_ratios(self):
        """tts_resample_segments_max_ratios: the most distinct ratios below 1 among the segments of one call."""
        return int(self.lib.tts_resample_segments_max_ratios())

    def resample_segments_tile(self):
        """tts_resample_segments_tile: the output samples of a segment one workgroup writes."""
        return int(self.lib.tts_resample_segments_tile())

    def resample_segments_plan(self, shape, segments, n_samples=None):
        """tts_resample_segments_plan, host only: the lengths ``n_out`` (int64 (B,)) of the rows that ``segments`` -- a
        RESAMPLE_SEGMENT array or rows ``(row, first, samples, ratio)`` -- make of a batch of ``shape`` (B, n) whose rows hold
        ``n_samples`` samples (None: all n).  ValueError for a list tts_resample_segments refuses (``resample_segment_list``),
        raised before the library is reached."""
        if len(shape) != 2:
            raise ValueError('resample_segments_plan: the shape of a batch (B, n) is needed, got {!r}'.format(tuple(shape)))
        B, n = int(shape[0]), int(shape[1])
        q, ns, n_out, _count = resample_segment_list(segments, B, n, n_samples)
        out = np.zeros(B, dtype=np.int64)
        rc = self.lib.tts_resample_segments_plan(q.ctypes.data, q.shape[0], B, n, _int32_ptr(ns), out.ctypes.data_as(POINTER(c_int64)))
        self._host_plan_check(rc)
        assert (out == n_out).all(), (out, n_out)
        return out

    def resample_segments(self, wav, segments, n_samples=None, N_out=None):
        """tts_resample_segments: ``resample`` with a ratio that varies along the utterance, on ``wav`` (B, n) -- a host array,
        which is uploaded, or a device buffer, which is read in place.  ``segments``: a RESAMPLE_SEGMENT array or rows ``(row,
        first, samples, ratio)``, the segments of a row one behind the other and the rows in order: source samples [first, first +
        samples) of the row at ``ratio`` output samples per input sample -- 1.0 exactly: copied bit for bit; otherwise
        tts_resample's windowed sinc with its position measured from ``first``, the taps reaching over the segment's borders into
        the row.  ``n_samples``: B lengths (host integers) -- samples at or behind them are never read; None: all n.
        include/sstts_hip.h has the definition.

        Returns ``(out, n_out)``: a fresh device array (B, N_out) and the int64 host lengths (B,) -- row b holds n_out[b] samples
        followed by +0.0.  ``N_out`` None: the largest length (at least 1).  ValueError for what the library refuses, raised
        before it is reached."""
        if len(wav.shape) != 2 or min(wav.shape) < 1:
            raise ValueError('resample_segments: a non-empty batch (B, n) is needed, got shape {}'.format(tuple(wav.shape)))
        B, n = (int(d) for d in wav.shape)
        q, ns, n_out, _count = resample_segment_list(segments, B, n, n_samples)
        longest = int(n_out.max())
        if N_out is None:
            N_out = max(longest, 1)
        if int(N_out) != N_out or not max(longest, 1) <= N_out <= RESAMPLE_SEGMENTS_MAX_N_OUT:
            raise ValueError('resample_segments: N_out = {!r} is not in max(n_out.max(), 1) = {} .. 2^30'.format(N_out, max(longest, 1)))
        p_wav, _k = self._in(wav, np.float32)
        out = self.empty((B, int(N_out)))
        got = np.zeros(B, dtype=np.int32)
        self._check_or_free(self.lib.tts_resample_segments(self.handle, p_wav, B, n, _int32_ptr(ns), q.ctypes.data, q.shape[0], int(N_out),
                                                           out.data_ptr(), _int32_ptr(got)), out)
        assert (got == n_out).all(), (got, n_out)
        return out, n_out

    def pitch_shift(self, wavs, sampling_rate, octaves, n_iter=25, seed=0, preserve_formants=False, order=None, init_phase=None):
        """The reference's waveform effect pitch_shift (audio/effects.py:9-43) as a composition of existing calls:
        ``time_stretch(wavs, rate)`` with rate = 2 ** -octaves, then ``resample`` from sampling_rate / rate back to
        sampling_rate, cut or zero-padded to the input's length (librosa's fix_length).  ``wavs``: one waveform (n,) or a
        uniform batch (B, n).  Returns a device array of the input's shape.

        ``preserve_formants`` (no reference counterpart): ``stft_magnitude`` (n_fft 1024, window 1024, hop 256, power 1),
        ``shift_magnitudes`` with one segment per row at ``shift_step(12 * octaves)`` for the fine structure and 65536 for the
        envelope (``order`` None: ``shift_order(sampling_rate)``), then ``griffin_lim`` at the same length: nothing is resampled,
        the 256 (n // 256) samples are zero-padded to the input's length.  ``init_phase`` (B, 513, 1 + n // 256): Griffin-Lim's
        initial phases in [0, 1) in place of the seed's."""
        o = pitch_octaves_value(octaves)
        if o is None:
            raise ValueError('pitch_shift: a shift in [-1, 1] octaves is needed')
        if preserve_formants:
            sr = float(sampling_rate)
            if not sr > 0:
                raise ValueError('pitch_shift: sampling_rate must be positive, got {!r}'.format(sampling_rate))
            wavs, single, B, n = _waveforms('pitch_shift', wavs, uniform=True)
            n_fft, win, hop = 1024, 1024, 256
            T = 1 + n // hop
            if hop * (T - 1) <= n_fft // 2:
                raise ValueError('pitch_shift: {} samples are a signal shorter than n_fft / 2'.format(n))
            step = shift_step(12.0 * o)
            mag = self.stft_magnitude(wavs, n_fft, win, hop, 1.0)
            shifted = wav = None
            try:
                shifted = self.shift_magnitudes(mag, [(b, 0, T, step, SHIFT_UNITY) for b in range(B)],
                                                order=shift_order(sr) if order is None else order)
                wav, _mse = self.griffin_lim(shifted, int(n_iter), win, hop, n_fft, init_phase=init_phase, seed=seed, want_mse=False)
                out, _n = self.resample_segments(wav, [(b, 0, hop * (T - 1), 1.0) for b in range(B)], N_out=n)   # (copies, then +0.0)
            finally:
                for a in (mag, shifted, wav):
                    if a is not None:
                        a.free()
            if single:
                out.shape = (n,)
            return out
        rate = float(np.exp2(-np.float64(o)))
        sr = float(sampling_rate)
        if not sr > 0:
            raise ValueError('pitch_shift: sampling_rate must be positive, got {!r}'.format(sampling_rate))
        single = len(wavs.shape) == 1
        n = int(wavs.shape[-1])
        st = self.time_stretch(wavs, rate, n_iter=n_iter, seed=seed)
        if single:
            st.shape = (1, st.shape[0])
        try:
            out = self.resample(st, sr / (sr / rate), N_out=n)
        finally:
            st.free()   # (tts_free waits for the device: the resampling that reads it has run)
        if single:
            out.shape = (n,)
        return out

    def synthesize(self, ids, n_steps, ref_db, max_db, power, n_iter, win_length, hop_length, init_phase=None,
                   seed=0, peak_normalize=True, want_mel=False, want_alignments=False, want_linear=False, wav=None,
                   momentum=None, stop_at_silence=None, speaking_rate=None, pitch=None, phase_init=None, loudness=None,
                   alignment_stats=None, limiter=None, token_times=None, equalizer=None, compressor=None, watermark=None, **refused):
        """tts_synthesize: ids -> waveforms in one call, everything on the device.  The settings from ``momentum`` to ``watermark``
        hold for this call alone, as SETTINGS has them.  ``output`` is ``synthesize_host``'s: this call's rows stay on the device,
        where ``resample`` and ``encode`` take them."""
        for row in SETTINGS:
            if row.host_only and row.keyword in refused:
                raise ValueError('synthesize: no {}= here -- the waveforms stay on the device as float32; resample and encode them '
                                 'there with Engine.resample and Engine.encode, or call synthesize_host'.format(row.keyword))
        if refused:
            raise TypeError('synthesize() got an unexpected keyword argument {!r}'.format(sorted(refused)[0]))
        call = self._settings(momentum=momentum, stop_at_silence=stop_at_silence, speaking_rate=speaking_rate, pitch=pitch,
                              phase_init=phase_init, loudness=loudness, alignment_stats=alignment_stats, limiter=limiter,
                              token_times=token_times, watermark=watermark, compressor=compressor, equalizer=equalizer)
        B, Ts = ids.shape
        T = n_steps * self.cfg.reduction
        r_call, o_call = call['speaking_rate'], call['pitch']
        # (without init_phase the pitch changes no shape here, and a product of rate and 2 ** -pitch outside [0.25, 4] is the
        #  library's to refuse, at the call)
        T_wav, T_init = synth_frame_counts(T, r_call, o_call if init_phase is not None else 0.0)
        F = 1 + self.cfg.n_fft // 2
        sp = TtsSynthParams(n_steps, ref_db, max_db, power, n_iter, win_length, hop_length, seed,
                            1 if peak_normalize else 0)
        self._check_ids(ids)
        p_ids, _k1 = self._in(ids, np.int32, 'ids')
        p_init, _k2 = self._in(init_phase, np.float32, 'init_phase')
        if init_phase is not None and int(np.prod(init_phase.shape)) != B * F * T_init:
            raise ValueError('synthesize: init_phase of shape {} given, {} needed'.format(tuple(init_phase.shape), (B, F, T_init)))
        if wav is not None and int(np.prod(wav.shape)) != B * hop_length * (T_wav - 1):
            raise ValueError('synthesize: wav buffer of shape {} given, {} needed'.format(tuple(wav.shape), (B, hop_length * (T_wav - 1))))
        wav = wav if wav is not None else self.empty((B, hop_length * (T_wav - 1)))
        # want_*: False, True (a fresh buffer) or a device array of the right size to write into (no allocation in the call)
        def _out(want, shape):
            if want is None or want is False:
                return None
            if want is True:
                return self.empty(shape)
            if int(np.prod(want.shape)) != int(np.prod(shape)):
                raise ValueError('synthesize: output buffer of shape {} given, {} needed'.format(want.shape, shape))
            return want
        mel = _out(want_mel, (B, T, self.cfg.n_mels))
        ali = _out(want_alignments, (n_steps, B, Ts))
        lin = _out(want_linear, (B, T, F))
        with call:
            self._check(self.lib.tts_synthesize(self.handle, p_ids, B, Ts, byref(sp), p_init, wav.data_ptr(),
                                                mel.data_ptr() if mel is not None else None,
                                                ali.data_ptr() if ali is not None else None,
                                                lin.data_ptr() if lin is not None else None))
        out = dict(wav=wav, mel=mel, alignments=ali, linear=lin)
        if call['stop_at_silence'][0]:
            out['n_frames'] = self.synth_frames(B)
        if call['token_times'][0]:
            self._token_times_Ts = Ts   # (what synth_token_times sizes its rows by)
        return out

    def synth_frames(self, B):
        """tts_synth_frames: the B frame counts (int32 host array) of the last ``synthesize`` / ``synthesize_host`` call made
        on the handle -- all T for a call made without end-of-speech stopping."""
        n_frames = np.zeros(int(B), dtype=np.int32)
        self._check(self.lib.tts_synth_frames(self.handle, _int32_ptr(n_frames), int(B)))
        return n_frames

    def synthesize_host(self, ids, n_steps, ref_db, max_db, power, n_iter, win_length, hop_length, seed=0,
                        peak_normalize=True, want_linear=False, want_alignments=False, momentum=None, stop_at_silence=None,
                        speaking_rate=None, pitch=None, phase_init=None, loudness=None, alignment_stats=None, limiter=None,
                        output=None, token_times=None, equalizer=None, compressor=None, watermark=None):
        """Asynchronous end-to-end call on HOST ids (int32 (B, T_sent)): returns a ticket at once; the upload, the
        network, Griffin-Lim and the download of the waveforms into pinned memory overlap with the neighbouring
        calls.  Keep at most three calls in flight: submit k + 2, then ``wait_host(ticket_k)``.
        The settings from ``momentum`` on hold for this call alone, as SETTINGS has them: they are read when the call is
        made, not when its work runs.  A call made with an ``output`` is fetched with ``wait_host_encoded``, not ``wait_host``.  A call that stops at silence returns once its post-net has run (the lengths:
        ``wait_host_frames``); the alignment records travel with the waveforms (``wait_host_alignment_stats``), and so do the
        timing marks of a call made with ``token_times`` (``wait_host_token_times``)."""
        call = self._settings(momentum=momentum, stop_at_silence=stop_at_silence, speaking_rate=speaking_rate, pitch=pitch,
                              phase_init=phase_init, loudness=loudness, alignment_stats=alignment_stats, limiter=limiter, output=output,
                              token_times=token_times, watermark=watermark, compressor=compressor, equalizer=equalizer)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        self._check_ids(ids)
        B, Ts = ids.shape
        sp = TtsSynthParams(n_steps, ref_db, max_db, power, n_iter, win_length, hop_length, seed, 1 if peak_normalize else 0,
                            (1 if want_linear else 0) | (2 if want_alignments else 0))
        t = c_int(-1)
        T_wav, _T_gl = synth_frame_counts(n_steps * self.cfg.reduction, call['speaking_rate'], 0.0)   # (the pitch changes no shape)
        with call:
            self._check(self.lib.tts_synthesize_host(self.handle, ids.ctypes.data, B, Ts, byref(sp), byref(t)))
        if call['token_times'][0]:
            self._token_times_Ts = Ts
        self._host_shapes[t.value] = (B, hop_length * (T_wav - 1))
        self._host_out_shapes[t.value] = ((B, n_steps * self.cfg.reduction, 1 + self.cfg.n_fft // 2), (n_steps, B, Ts))
        return t.value

    def wait_host_outputs(self, ticket, copy=True):
        """(linear (B, T, F) or None, alignments (n_steps, B, Ts) or None) of a ``synthesize_host`` call made with
        ``want_linear`` / ``want_alignments``; views of pinned buffers with the waveform buffer's lifetime unless ``copy``.
        Call it BEFORE ``wait_host`` of the same ticket or keep the shapes yourself (it does not consume the ticket)."""
        pl, pa = c_void_p(), c_void_p()
        nl, na = c_size_t(0), c_size_t(0)
        self._check(self.lib.tts_wait_host_outputs(self.handle, int(ticket), byref(pl), byref(nl), byref(pa), byref(na)))
        shl, sha = self._host_out_shapes.pop(ticket, ((nl.value,), (na.value,)))
        lin = np.ctypeslib.as_array(ctypes.cast(pl, POINTER(c_float)), shape=(nl.value,)).reshape(shl) if nl.value else None
        ali = np.ctypeslib.as_array(ctypes.cast(pa, POINTER(c_float)), shape=(na.value,)).reshape(sha) if na.value else None
        if copy:
            lin = None if lin is None else lin.copy()
            ali = None if ali is None else ali.copy()
        return lin, ali

    def wait_host_frames(self, ticket):
        """The B frame counts (int32, a copy) of a ``synthesize_host`` call: tts_wait_host_frames.  Waits like ``wait_host``
        and does not consume the ticket; all T for a call made without ``stop_at_silence``."""
        p = c_void_p()
        n = c_int(0)
        self._check(self.lib.tts_wait_host_frames(self.handle, int(ticket), byref(p), byref(n)))
        if not n.value:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(ctypes.cast(p, POINTER(c_int32)), shape=(n.value,)).copy()

    def wait_host_encoded(self, ticket, copy=True):
        """tts_wait_host_encoded: ``(codes, n_samples, stats)`` of a ``synthesize_host`` call made with an ``output``: the codes
        (B, N_out) as int16 ('pcm16'), uint8 ('pcm8', 'mulaw', 'alaw') or float32 ('float32' at another rate), the samples each
        row holds (int32 (B,): behind them the row is the format's silence) and the encoder's records ((B,) of
        ``ENCODE_RECORD``; None for float32).  ``copy=False``: the codes are a view of the library's pinned buffer, valid until
        the THIRD ``synthesize_host`` call after the one that produced it."""
        data, held, st = c_void_p(), c_void_p(), c_void_p()
        nbytes = c_size_t(0)
        fmt, N_out, B = c_int(0), c_int(0), c_int(0)
        self._check(self.lib.tts_wait_host_encoded(self.handle, int(ticket), byref(data), byref(nbytes), byref(fmt), byref(N_out), byref(held),
                                                   byref(st), byref(B)))
        self._host_shapes.pop(ticket, None)
        raw = np.ctypeslib.as_array(ctypes.cast(data, POINTER(ctypes.c_uint8)), shape=(nbytes.value,))
        codes = raw.view(FORMAT_DTYPES[fmt.value]).reshape(B.value, N_out.value)
        n_samples = np.ctypeslib.as_array(ctypes.cast(held, POINTER(c_int32)), shape=(B.value,)).copy()
        stats = None
        if st.value:
            stats = np.ctypeslib.as_array(ctypes.cast(st, POINTER(c_int32)), shape=(B.value * 4,)).copy().view(ENCODE_RECORD).reshape(B.value)
        return (codes.copy() if copy else codes), n_samples, stats

    def wait_host(self, ticket, copy=True):
        """Waveforms (B, hop*(T-1)) float32 of a ``synthesize_host`` call.  ``copy=False`` returns a view of the library's
        pinned buffer, valid until the THIRD ``synthesize_host`` call (three buffer sets) after the one that produced it."""
        p = c_void_p()
        n = c_size_t(0)
        self._check(self.lib.tts_wait_host(self.handle, int(ticket), byref(p), byref(n)))
        shape = self._host_shapes.pop(ticket, (n.value,))
        view = np.ctypeslib.as_array(ctypes.cast(p, POINTER(c_float)), shape=(n.value,)).reshape(shape)
        return view.copy() if copy else view

    def stft(self, wav, n_fft, win_length, hop_length):
        """complex64 (B, F, n_frames) = librosa.stft per utterance."""
        B, n = wav.shape
        p_wav, _k = self._in(wav, np.float32)
        Tf = 1 + n // hop_length
        out = self.empty((B, 1 + n_fft // 2, Tf), np.complex64)
        self._check(self.lib.tts_stft(self.handle, p_wav, B, n, n_fft, win_length, hop_length, out.data_ptr()))
        return out

    def stft_magnitude(self, wav, n_fft, win_length, hop_length, power=1.0):
        B, n = wav.shape
        p_wav, _k = self._in(wav, np.float32)
        Tf = 1 + n // hop_length
        out = self.empty((B, 1 + n_fft // 2, Tf))
        self._check(self.lib.tts_stft_magnitude(self.handle, p_wav, B, n, n_fft, win_length, hop_length, power,
                                                out.data_ptr()))
        return out

    def mel_spectrogram(self, lin, n_fft, sampling_rate, n_mels, fmin, fmax):
        B, F, Tf = lin.shape
        p_lin, _k = self._in(lin, np.float32)
        out = self.empty((B, n_mels, Tf))
        self._check(self.lib.tts_mel_spectrogram(self.handle, p_lin, B, Tf, n_fft, sampling_rate, n_mels, fmin,
                                                 fmax if fmax is not None else 0.0, out.data_ptr()))
        return out

    def db_convert(self, x, mode, ref_db=0.0, max_db=0.0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        d = self.to_device(x)
        self._check(self.lib.tts_db_convert(self.handle, d.ptr, x.size, mode, ref_db, max_db, d.ptr))
        return d.to_host()

    # ------------------------------------------------------------------ dataset features
    def feature_params(self, **kw):
        """tts_default_feature_params with fields overridden by keyword (names of struct tts_feature_params)."""
        p = TtsFeatureParams()
        self._check(self.lib.tts_default_feature_params(byref(p)))
        for k, v in kw.items():
            if k == 'struct_size' or not hasattr(p, k):
                raise TypeError('unknown feature parameter {!r}'.format(k))
            setattr(p, k, v)
        return p

    @staticmethod
    def _ragged(wavs):
        wavs = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in wavs]
        if not wavs:
            raise ValueError('no recordings')
        offsets = np.zeros(len(wavs) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([w.size for w in wavs])
        return np.concatenate(wavs), offsets

    def trim_bounds(self, wavs, frame_length=2048, hop_length=512, top_db=60.0):
        """librosa.effects.trim (0.6) interval of every recording of a list of 1-D float32 arrays: int64 (B, 2) {start, end}."""
        flat, offsets = self._ragged(wavs)
        B = len(wavs)
        d = self.to_device(flat)
        bounds = self.empty((B, 2), np.int64)
        self._check(self.lib.tts_trim_bounds(self.handle, d.ptr, offsets.ctypes.data, B, int(frame_length), int(hop_length),
                                             float(top_db), bounds.data_ptr()))
        return bounds.to_host()

    def extract_features(self, wavs, params=None):
        """Features of a list of 1-D float32 recordings (tts_plan_features + tts_extract_features, one batch):
        a list of (mel (T_red, n_mels r), lin (T_red, F r)) float32 arrays, as the reference's load_audio returns them."""
        p = params if params is not None else self.feature_params()
        flat, offsets = self._ragged(wavs)
        B = len(wavs)
        d = self.to_device(flat)
        plan = np.zeros(3 * B, dtype=np.int64)
        self._check(self.lib.tts_plan_features(self.handle, d.ptr, offsets.ctypes.data, B, byref(p), plan.ctypes.data))
        plan = plan.reshape(B, 3)
        rows = int(plan[:, 2].sum())
        F = 1 + p.n_fft // 2
        mel = self.empty((rows, p.n_mels))
        lin = self.empty((rows, F))
        self._check(self.lib.tts_extract_features(self.handle, d.ptr, offsets.ctypes.data, B, byref(p),
                                                  plan.ctypes.data, mel.data_ptr(), lin.data_ptr()))
        mel_h, lin_h = mel.to_host(), lin.to_host()
        out, r0, r = [], 0, p.reduction
        for b in range(B):
            tp = int(plan[b, 2])
            out.append((mel_h[r0:r0 + tp].reshape(tp // r, p.n_mels * r), lin_h[r0:r0 + tp].reshape(tp // r, F * r)))
            r0 += tp
        self.last_feature_plan = plan
        return out

    # ------------------------------------------------------------------ profiling / debug
    def profile_reset(self):
        self._check(self.lib.tts_profile_reset(self.handle))

    def decoder_kernel_choice(self, B, Ts, pipelined=True):
        """0 launch per layer, 1 persistent (streamed weights), 2 persistent (weight-stationary): what a call of this shape takes"""
        rc = self.lib.tts_decoder_kernel_choice(self.handle, int(B), int(Ts), 1 if pipelined else 0)
        if rc < 0:
            self._check(rc)
        return rc

    def device_info(self):
        """(uuid as 32 hex digits, compute units) of the handle's device"""
        buf = ctypes.create_string_buffer(33)
        n = c_int()
        self._check(self.lib.tts_device_info(self.handle, buf, byref(n)))
        return buf.value.decode(), n.value

    def profile_get(self, stage):
        ms = c_float()
        n = c_int64()
        self._check(self.lib.tts_profile_get(self.handle, stage.encode(), byref(ms), byref(n)))
        return ms.value, n.value

    def debug_workspace(self, name, shape, dtype=np.float32):
        p = c_void_p()
        nb = c_size_t()
        self._check(self.lib.tts_debug_workspace(self.handle, name.encode(), byref(p), byref(nb)))
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= nb.value, (name, out.nbytes, nb.value)
        self._check(self.lib.tts_memcpy_d2h(self.handle, out.ctypes.data, p, out.nbytes))
        return out

    def debug_workspace_extent(self, name):
        """(device pointer, bytes) of a workspace as it stands now; nothing is copied"""
        p, nb = c_void_p(), c_size_t()
        self._check(self.lib.tts_debug_workspace(self.handle, name.encode(), byref(p), byref(nb)))
        return p.value, nb.value
