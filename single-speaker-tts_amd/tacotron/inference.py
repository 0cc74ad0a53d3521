"""Drop-in mirror of the reference's ``tacotron.inference`` (tacotron/inference.py).

``pad_sentence`` (:22-27), ``inference(model, sentences)`` (:30-105) and the body of
``__main__`` (:130-200) as :func:`synthesize_sentences`: ids -> padded batch -> network ->
de-normalise -> ``** magnitude_power`` -> Griffin-Lim -> ``{i+1}.wav``.

Where the reference fans Griffin-Lim out to 6 worker processes, one utterance each
(:185-188), the whole batch is reconstructed by one batched kernel sequence on the GPU.
"""
import functools
import inspect
import json
import logging
import os
import types

import numpy as np

from . import attention_check, marks as marks_, prosody
from .._hip import (ALIGNMENT_RECORD, FMT_F32, FORMAT_NAMES, JOIN_MAX_FADE, LIMIT_LOOKAHEAD_MS, LOUDNESS_MAX_PEAK, RESAMPLE_SEGMENTS_MAX_RATIOS, shift_step,
                    compressor_params, compressor_setting, watermark_setting, equalizer_sections, equalizer_setting, limiter_lookahead, limiter_setting, loudness_setting, momentum_thousandths, output_is_on, output_ratio,
                    output_setting, phase_init_value, pitch_octaves_value, pitch_semitones_value, resampled_length,
                    silence_keep_frames, speaking_rate_value, stop_at_silence_setting, synth_frame_counts, token_times_jump)
from ..audio.conversion import ms_to_samples
from ..audio.io import save_wav
from ..datasets.text_split import BREAKS, MAX_CHARS, abbreviations_of, split_text, split_text_spans
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
    hp = getattr(hp, 'hparams', hp) or model_params   # (a model serves for its hyper-parameters, None for the default ones)
    hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    return stop_at_silence_setting((stop_at_silence_db, silence_keep_frames(ms_to_samples(float(silence_keep_ms), hp.sampling_rate), hop)))


def cut_waveforms(wavs, n_frames, hop):
    """Row b of a padded batch cut to its own hop (n_frames[b] - 1) samples: a list of arrays."""
    return [wavs[b][:hop * (int(n_frames[b]) - 1)] for b in range(len(n_frames))]


def pad_id():
    """the id the sentences are padded with (``pad_sentence``): what the attention diagnostics take the sentence lengths from"""
    return int(dataset_params.vocabulary_dict['pad'])


log = logging.getLogger(__name__)


def output_of(hp, output):
    """``output`` of the helpers below -- None, a format name ('pcm16', 'pcm8', 'mulaw', 'alaw', 'float32') or ``(format, dither,
    rate_out)`` with ``dither`` 'tpdf' or None and ``rate_out`` in Hz or None (the model's rate) -- as the engine's checked
    ``output`` at the model's sampling rate (``_hip.output_setting``), or None where it changes nothing.  A bare name is dithered
    and keeps the rate.  ValueError for anything else."""
    if output is None:
        return None
    if isinstance(output, (tuple, list)):
        if len(output) != 3:
            raise ValueError('output must be None, a format name or (format, dither, rate_out), got {!r}'.format(output))
        fmt, dither, rate_out = output
    else:
        fmt, dither, rate_out = output, 'tpdf', None
    rate_in = int(getattr(hp, 'hparams', hp).sampling_rate)
    setting = output_setting((fmt, dither, rate_in, rate_in if rate_out is None else rate_out))
    return setting if output_is_on(setting) else None


def output_rate(hp, setting):
    """the sampling rate of what a checked ``output`` (``output_of``) delivers"""
    return int(getattr(hp, 'hparams', hp).sampling_rate) if setting is None or setting[2] == setting[3] else setting[3]


def output_encoding(setting):
    """the ``encoding`` ``audio.io.save_wav`` takes for what a checked ``output`` delivers"""
    return 'float32' if setting is None else FORMAT_NAMES[setting[0]]


def log_clipped(stats, first=0, what='utterance'):
    """one line per row whose record counts clipped samples"""
    for b, rec in enumerate(() if stats is None else stats):
        if rec['clipped'] > 0:
            log.warning('%s %d: %d of %d samples clipped in the encoder (leave head room: a limiter at -1 dB)', what, first + b + 1,
                        int(rec['clipped']), int(rec['n']))


def deliver_rows(engine, rows, lengths, setting, seed=0, first=0, what='utterance'):
    """Device rows (B, N) float32, each holding ``lengths[b]`` samples (None: all N), in the delivery format of a checked
    ``output``: ``Engine.resample`` where the rates differ, then ``Engine.encode`` with the dither's ``seed``, on the device.
    Returns the codes as host arrays -- a list of B rows cut to what they hold where ``lengths`` is given, else one (B, N') array --
    and logs every row that clipped.  ``rows`` is left as it was."""
    ratio = output_ratio(setting)
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    work = rows
    if ratio != 1.0:
        N_out = resampled_length(int(rows.shape[-1]), ratio)
        work = engine.resample(rows, ratio, n_samples=lens, N_out=N_out)
        if lens is not None:
            lens = np.array([resampled_length(int(n), ratio) for n in lens], dtype=np.int32)
    try:
        if setting[0] != FMT_F32:
            codes, stats = engine.encode(work, setting[0], dither=setting[1], seed=seed, n_samples=lens)
            host = codes.to_host()
            codes.free()
            log_clipped(stats, first, what)
        else:
            host = work.to_host()
    finally:
        if work is not rows:
            work.free()
    if host.ndim == 1:
        host = host[None]
    return host if lens is None else [host[b, :int(n)] for b, n in enumerate(lens)]


def deliver(engine, wavs, setting, seed=0, norm=False, what='utterance'):
    """Host waveforms -- a list of float32 arrays of any lengths -- in the delivery format of a checked ``output``: padded to one
    batch, uploaded, peak-normalised row by row with ``norm``, then ``deliver_rows``.  Returns the list of code arrays; an empty
    waveform stays empty."""
    wavs = [np.asarray(w, dtype=np.float32) for w in wavs]
    kept = [b for b, w in enumerate(wavs) if len(w)]
    dtype = np.float32 if setting[0] == FMT_F32 else (np.int16 if FORMAT_NAMES[setting[0]] == 'pcm16' else np.uint8)
    out = [np.zeros(0, dtype=dtype) for _ in wavs]
    if kept:
        lens = np.array([len(wavs[b]) for b in kept], dtype=np.int32)
        batch = np.zeros((len(kept), int(lens.max())), dtype=np.float32)
        for r, b in enumerate(kept):
            batch[r, :lens[r]] = wavs[b]
        rows = engine.to_device(batch)
        try:
            if norm:
                engine.peak_normalize(rows)
            for b, codes in zip(kept, deliver_rows(engine, rows, lens, setting, seed, 0, what)):
                out[b] = codes
        finally:
            rows.free()
    return out


class SynthSettings(object):
    """The synthesis settings every helper of this layer takes, checked once -- ValueError before an engine is touched, in the
    order of ``_hip.SETTINGS`` -- and kept as the checked values ``momentum``, ``stop``, ``rate``, ``octaves``, ``phase_init``,
    ``loud``, ``check_alignment``, ``limiter``, ``output`` (``output_of``), ``watermark``, ``compressor`` and ``equalizer``.  ``hp``: the hyper-parameters the stopping takes its hop from, or a model that has them.

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
    ``attention_check.verdict`` of every utterance, an empty tuple where the attention read the sentence cleanly.
    ``limiter``: None (the engine's setting), a ceiling or ``(ceiling, lookahead_ms, oversample)`` -- a look-ahead peak limiter
    (``Engine.limit``) runs last over every utterance on the device, behind the loudness gain or the peak normalisation: no
    sample ends above the ceiling, and what never was keeps its bits.  A bare ceiling looks 5 ms ahead at the interpolated
    (true) peaks.
    ``output``: None (float32 at the model's rate), a format name -- 'pcm16', 'pcm8', 'mulaw', 'alaw' -- or ``(format, dither,
    rate_out)``: what the helper hands back (and writes) is in that sample format and at that rate, resampled and encoded on the
    device behind everything else (``Engine.resample``, ``Engine.encode``: TPDF dither unless ``dither`` is None, saturation;
    a row that clipped is logged with its count).  The resampler can overshoot a limiter's ceiling: leave head room.
    ``marks``: None, 'word' or 'char' -- the call also searches its alignments for the best monotone path on the device
    (``Engine.token_times``, at most ``marks_max_jump`` tokens a decoder step; 4, untuned) and the helper answers with timing
    marks as its last element (``tacotron.marks``): when every word -- and with 'char' every character -- is spoken, in
    milliseconds and in samples of what is delivered.
    ``watermark``: None (the engine's setting), a key, ``(key, payload)`` or ``(key, payload, payload_bits, chip, chips_per_symbol,
    strength)``: a keyed spread-spectrum carrier (``Engine.watermark_embed``) is added under the local envelope of every utterance;
    ``audio.metrics.detect_watermark`` finds it.  The defaults (16 bits, 8 samples a chip, 64 chips a symbol, 0.02 of the envelope)
    are UNTUNED: nobody has listened.
    ``compressor``: None (the engine's setting), a profile name -- 'speech', 'telephony', 'small-speaker'; every preset is untuned
    -- or ``(threshold_db, ratio[, knee_db[, attack_ms[, release_ms[, makeup_db]]]])``: a feed-forward peak compressor
    (``Engine.compress``) lowers the crest factor of every utterance.
    ``equalizer``: None (the engine's setting), a profile name -- 'telephony', 'small-speaker', 'rumble', 'bright', 'warm'; every
    preset is untuned -- a list of ``(kind, f0_hz[, q[, gain_db]])`` sections (kinds 'lowpass', 'highpass', 'peak', 'lowshelf',
    'highshelf') or an (S, 5) array of second-order sections: a cascade of up to 8 biquads (``Engine.equalize``) shapes the
    spectrum of every utterance; refused where a corner does not fit the model's sampling rate.
    The last three run on the device behind Griffin-Lim, the pitch and the peak normalisation -- the equaliser, then the compressor,
    then the watermark -- and ahead of the loudness gain and the limiter.  Lengths and timing marks do not change (the equaliser's
    group delay of a few samples is ignored).  A boost or a make-up gain behind the peak normalisation can pass 1.0: give it a
    limiter or a loudness target."""

    def __init__(self, hp, momentum=0.0, stop_at_silence_db=None, silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0,
                 phase_init='random', loudness=None, check_alignment=False, pitch_semitones=None, limiter=None, output=None,
                 marks=None, marks_max_jump=4, watermark=None, compressor=None, equalizer=None):
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
        self.limiter = limiter_setting(limiter)
        self.output = output_of(hp, output)
        self.marks = marks_.marks_kind(marks)
        self.marks_max_jump = token_times_jump(marks_max_jump, 'marks_max_jump')
        self.watermark = watermark_setting(watermark)
        self.compressor = compressor_setting(compressor)
        self.equalizer = equalizer_setting(equalizer)
        rate = getattr(getattr(hp, 'hparams', hp), 'sampling_rate', None)   # (the coefficients, where the model's rate is known)
        if self.compressor is not None and rate:
            compressor_params(self.compressor, int(rate))
        if self.equalizer is not None and rate:
            equalizer_sections(self.equalizer, int(rate))

    def engine_keywords(self):
        """the settings as ``Engine.synthesize`` / ``Engine.synthesize_host`` take them"""
        return dict(momentum=self.momentum, stop_at_silence=self.stop, speaking_rate=self.rate, pitch=self.octaves,
                    phase_init=self.phase_init, loudness=self.loud, alignment_stats=(True, pad_id()) if self.check_alignment else None,
                    limiter=self.limiter, token_times=(True, pad_id(), self.marks_max_jump) if self.marks else None,
                    watermark=self.watermark, compressor=self.compressor, equalizer=self.equalizer)

    def host_keywords(self):
        """... and as ``Engine.synthesize_host`` alone takes them: with the delivery format"""
        return dict(self.engine_keywords(), output=self.output)

    def keywords(self):
        """the settings as the stand-alone stages honour them (``serve.post_process_spectrograms``): the checked values, without
        ``check_alignment``, ``output`` and the marks"""
        return dict(momentum=self.momentum, stop_at_silence_db=self.stop_at_silence_db, silence_keep_ms=self.silence_keep_ms,
                    speaking_rate=self.rate, pitch=self.octaves, phase_init=self.phase_init, loudness=self.loud, limiter=self.limiter,
                    watermark=self.watermark, compressor=self.compressor, equalizer=self.equalizer)

    def file_norm(self):
        """the peak normalisation of the file helpers, ``(on the device, in save_wav)``: none with a loudness or a limiter, else
        ahead of the encoder where there is an ``output`` and on the way to the disk where the files are float32"""
        norm = self.loud is None and self.limiter is None
        return norm and self.output is not None, norm and self.output is None


SETTING_KEYWORDS = tuple(inspect.signature(SynthSettings.__init__).parameters)[2:]


def takes_settings(*refuses, only=None):
    """Makes a helper of this layer out of a function that takes ``**settings`` -- the keywords of ``SynthSettings``, all but
    ``refuses`` or ``only`` those named -- and returns the parts of its answer by name, a dict (a generator: yields one per item).
    The helper refuses the keywords it does not take as Python would (TypeError) and answers in the public form its docstring
    states: the waveforms bare where they are the only part, else a tuple of the parts in the order they were put in.  The
    callers inside this layer read the parts, from ``helper.parts``, the function itself; ``inspect.signature(helper)`` lists the
    keywords the helper takes, with the record's defaults, in place of ``**settings``."""
    if only is not None:
        refuses = tuple(k for k in SETTING_KEYWORDS if k not in only)

    def make(parts):
        def taken(keywords):
            for k in refuses:
                if k in keywords:
                    raise TypeError("{}() got an unexpected keyword argument '{}'".format(parts.__name__, k))
            return keywords

        def answer(named):
            return tuple(named.values()) if len(named) > 1 else named['wavs']

        if inspect.isgeneratorfunction(parts):
            def helper(*args, **keywords):
                for named in parts(*args, **taken(keywords)):
                    yield answer(named)
        else:
            def helper(*args, **keywords):
                return answer(parts(*args, **taken(keywords)))
        functools.update_wrapper(helper, parts)
        own = [p for p in inspect.signature(parts).parameters.values() if p.kind is not p.VAR_KEYWORD]
        record = inspect.signature(SynthSettings.__init__).parameters
        helper.__signature__ = inspect.Signature(own + [record[k].replace(kind=inspect.Parameter.KEYWORD_ONLY)
                                                        for k in SETTING_KEYWORDS if k not in refuses])
        helper.parts = parts
        return helper
    return make


def call_constants(hp, n_steps=None, n_iter=None):
    """What the calls of this layer are made with, of a model or of hyper-parameters alone: ``win_len`` and ``hop`` in samples,
    the loader's dB pair, Griffin-Lim's ``n_iter`` and the decoder steps ``S`` (the model's unless given, None without a model)
    with their frames ``T``, and ``synth``: what ``Engine.synthesize`` and ``synthesize_host`` take behind the ids."""
    model, hp = hp, getattr(hp, 'hparams', hp)
    loader = dataset_params.dataset_loader
    c = types.SimpleNamespace(win_len=ms_to_samples(hp.win_len, hp.sampling_rate), hop=ms_to_samples(hp.win_hop, hp.sampling_rate),
                              ref_db=loader.mel_mag_ref_db, max_db=loader.mel_mag_max_db,
                              n_iter=hp.reconstruction_iterations if n_iter is None else n_iter,
                              S=n_steps or (model.n_steps() if hasattr(model, 'n_steps') else None))
    c.T = None if c.S is None else c.S * hp.reduction
    c.synth = (c.S, c.ref_db, c.max_db, hp.magnitude_power, c.n_iter, c.win_len, c.hop)
    return c


def held_samples(c, s, n_frames, B):
    """The samples each of a call's B rows holds at the model's rate, (B,) int64: hop (n_frames[b] - 1) of the frame counts a call
    with stopping reports, or (``n_frames`` None) the call's hop (T' - 1) in every row.  ``c``: the call's ``call_constants``."""
    if n_frames is None:
        n_frames = [synth_frame_counts(c.T, s.rate, 0.0)[0]] * B
    return c.hop * (np.asarray(n_frames, dtype=np.int64) - 1)


def finishing_tail(caller, s, sampling_rate, deliver=True):
    """The tail behind a Griffin-Lim that a helper composes of stand-alone stages.  The limiter's look-ahead becomes samples here,
    before an engine is touched (ValueError that names ``caller``); the function returned then runs, on device rows (B, N) that
    hold ``held[b]`` samples each (None: all N), a peak normalisation (``peak_normalize``, where there is no ``loudness``), the
    ``equalizer`` (its sections are made here too, at ``sampling_rate``), the ``compressor`` (its coefficients likewise; an
    engine's ``compress`` is not touched without one), the ``watermark`` (an engine's ``watermark_embed`` likewise), the ``loudness``,
    the ``limiter``,
    and hands back ``deliver_rows`` for an ``output`` (with ``deliver``; the dither's ``seed``) or else the rows downloaded, a list
    of B arrays cut to what they hold.  ``rows`` stays the caller's to free."""
    lookahead = None if s.limiter is None else limiter_lookahead(caller, s.limiter[1], sampling_rate)
    sections = None if s.equalizer is None else equalizer_sections(s.equalizer, sampling_rate)
    dynamics = None if s.compressor is None else ('params', compressor_params(s.compressor, sampling_rate))

    def finish(engine, rows, held, seed=0, peak_normalize=False):
        if s.loud is None and peak_normalize:
            engine.peak_normalize(rows)
        if sections is not None:
            engine.equalize(rows, sections, n_samples=held)
        if dynamics is not None:
            engine.compress(rows, dynamics, n_samples=held)
        if s.watermark is not None:
            engine.watermark_embed(rows, s.watermark, n_samples=held)
        if s.loud is not None:
            engine.loudness_normalize(rows, sampling_rate, s.loud[0], s.loud[1], n_samples=held)
        if s.limiter is not None:
            engine.limit(rows, s.limiter[0], lookahead, s.limiter[2], n_samples=held)
        if deliver and s.output is not None:
            return deliver_rows(engine, rows, held, s.output, seed)
        return list(rows.to_host()) if held is None else engine.download_rows(rows, held)
    return finish


def marks_of_batch(hp, s, ids, start, stats, n_held, wavs, mark_texts=None):
    """The timing marks of one call, a list of marks per row (``marks.marks_of_row``): ``start`` and ``stats`` as
    ``Engine.synth_token_times`` returns them, ``n_held`` the samples every row holds at the model's rate, ``wavs`` what is
    delivered (its lengths bound the marks' samples), ``s`` the call's ``SynthSettings``.  ``mark_texts``: per row ``(raw,
    processed, spans)`` for raw offsets (``marks.token_spans``); None: the processed characters of the ids (``marks.ids_text``)."""
    hp = getattr(hp, 'hparams', hp)
    hop = ms_to_samples(hp.win_hop, hp.sampling_rate)
    out = []
    for b in range(len(start)):
        if mark_texts is None:
            raw = None
            processed, spans = marks_.ids_text(ids[b], stats['n_sent'][b], dataset_params.vocabulary_dict)
        else:
            raw, processed, spans = mark_texts[b]
        out.append(marks_.marks_of_row(processed, spans, start[b], hp.reduction, hop, s.rate, int(n_held[b]), hp.sampling_rate,
                                       output_rate(hp, s.output), len(wavs[b]), s.marks, raw=raw, stats=stats[b]))
    return out


@takes_settings()
def synthesize_batch(model, sentences, n_steps=None, n_iter=None, init_phase=None, seed=0, peak_normalize=False, mark_texts=None,
                     **settings):
    """ids (B, T_sent) -> waveforms (B, hop*(T-1)) float32: inference() + the synthesize() closure
    of the reference (tacotron/inference.py:170-188) fused into one device call.  ``settings``: the keywords of
    ``SynthSettings``.  With ``stop_at_silence_db`` the result is a list of B waveforms, with ``check_alignment`` it is
    ``(waveforms, records, verdicts)``.  With an ``output`` the waveforms are that format's codes at its rate, made of the call's
    device rows (``deliver_rows``; the dither's seed is ``seed``).  With ``marks`` the result gains, as its last element, a list of
    timing marks per row -- of the processed characters of the ids, with offsets into that string (``mark_texts``: of raw texts)."""
    s = SynthSettings(model, **settings)
    c = call_constants(model, n_steps, n_iter)
    eng, B = model.engine, len(sentences)
    out = eng.synthesize(np.ascontiguousarray(sentences, dtype=np.int32), *c.synth, init_phase=init_phase, seed=seed,
                         peak_normalize=peak_normalize, **s.engine_keywords())
    n_frames = out['n_frames'] if s.stop is not None else None
    if s.output is not None:
        wavs = deliver_rows(eng, out['wav'], None if n_frames is None else held_samples(c, s, n_frames, B), s.output, seed)
    else:
        wavs = out['wav'].to_host() if n_frames is None else cut_waveforms(out['wav'].to_host(), n_frames, c.hop)
    parts = dict(wavs=wavs)
    if s.check_alignment:
        parts['records'] = eng.synth_alignment_stats(B)
        parts['verdicts'] = attention_check.verdict(parts['records'])
    if s.marks:
        start, stats = eng.synth_token_times(B)
        parts['marks'] = marks_of_batch(model, s, np.asarray(sentences), start, stats, held_samples(c, s, n_frames, B), wavs, mark_texts)
    return parts


@takes_settings()
def synthesize_stream(model, batches, n_steps=None, n_iter=None, seed=0, peak_normalize=False, copy=False, want_linear=False,
                      want_alignments=False, mark_texts=None, **settings):
    """Generator over batches of padded id sequences (each (B, T_sent) int32, HOST arrays) -> per batch the waveforms
    (B, hop*(T-1)) float32 in host memory, with THREE batches in flight: batch k + 2 is uploaded and encoded, batch k + 1
    is in its decoder, batch k in its post-net / Griffin-Lim while batch k - 1 is being downloaded (the reference runs the
    batches one after the other, tacotron/inference.py:75-101,185-200).  The arrays yielded are views of the library's
    pinned buffers unless ``copy``: valid until two more batches have been requested.

    With ``want_linear`` / ``want_alignments`` every item is a tuple ``(wavs, linear, alignments)``: the normalised linear
    spectrograms (B, T, 1025) -- what ``model.output_linear_spec`` is, the thing the reference's ``inference()`` fetches
    (:75-92) -- and the alignments (n_steps, B, T_sent) of the same call, downloaded behind the waveforms (None where not
    asked for).  ``settings``: the keywords of ``SynthSettings``.  With ``stop_at_silence_db`` the waveforms
    of a batch are a list of B arrays (views of the pinned rows unless ``copy``), each cut to its own length.  With
    ``check_alignment`` every item additionally carries the batch's alignment records and verdicts, ``(wavs, records,
    verdicts)`` or ``(wavs, linear, alignments, records, verdicts)``; the 56 bytes per utterance come down with the waveforms.
    With an ``output`` the call itself resamples and encodes its rows on the device (tts_set_output: the dither's seed is the
    call's) and only the codes are downloaded: the waveforms are int16 or uint8 arrays (float32 for 'float32' at another rate) at
    the output rate, cut to what each row holds with ``stop_at_silence_db``; a row that clipped is logged with its count.
    With ``marks`` every item is a tuple whose last element is the batch's timing marks, a list per row (of the processed
    characters of the ids -- or, with ``mark_texts``, an iterator that gives per batch what ``synthesize_batch`` takes by that name,
    of raw texts); the 4 T_sent + 36 bytes per utterance come down with the waveforms."""
    # (a generator: a bad setting is refused at its first item, before the engine is touched)
    s = SynthSettings(model, **settings)
    c = call_constants(model, n_steps, n_iter)
    eng = model.engine
    served = [0]   # utterances answered so far: what a clipped row is logged by

    def waveforms(ticket):
        if s.output is not None:
            codes, held, stats = eng.wait_host_encoded(ticket, copy=copy)
            log_clipped(stats, served[0])
            served[0] += len(held)
            return codes if s.stop is None else [codes[b, :int(n)] for b, n in enumerate(held)]
        if s.stop is None:
            return eng.wait_host(ticket, copy=copy)
        n_frames = eng.wait_host_frames(ticket)
        return cut_waveforms(eng.wait_host(ticket, copy=copy), n_frames, c.hop)

    def collect(ticket, ids, texts):
        records = eng.wait_host_alignment_stats(ticket) if s.check_alignment else None
        outputs = eng.wait_host_outputs(ticket, copy=copy) if want_linear or want_alignments else None
        parts = dict(wavs=waveforms(ticket))
        if outputs is not None:
            parts['linear'], parts['alignments'] = outputs
        if records is not None:
            parts['records'], parts['verdicts'] = records, attention_check.verdict(records)
        if s.marks:
            start, stats = eng.wait_host_token_times(ticket)
            held = held_samples(c, s, eng.wait_host_frames(ticket) if s.stop is not None else None, len(start))
            parts['marks'] = marks_of_batch(model, s, ids, start, stats, held, parts['wavs'], texts)
        return parts

    # three batches in flight (the library's three buffer sets): the encoder of batch k + 2 runs one inter-Griffin-Lim gap
    # ahead of its decoder, which follows the decoder of batch k + 1 without a pause, beside the Griffin-Lim of batch k
    pending = []   # (ticket, its ids, what its marks take of the raw texts)
    for k, ids in enumerate(batches):
        ticket = eng.synthesize_host(ids, *c.synth, seed=seed + k, peak_normalize=peak_normalize, want_linear=want_linear,
                                     want_alignments=want_alignments, **s.host_keywords())
        pending.append((ticket, np.asarray(ids), next(mark_texts) if s.marks and mark_texts is not None else None))
        if len(pending) == 3:
            yield collect(*pending.pop(0))
    while pending:
        yield collect(*pending.pop(0))


@takes_settings(only=('momentum', 'phase_init'))
def inference_stream(model, batches, n_steps=None, n_iter=None, seed=0, **settings):
    """``inference()`` over a stream of batches with three calls in flight: per batch ``(spectrograms, waveforms)`` where
    ``spectrograms`` is what the reference's ``inference()`` returns for that batch -- per utterance the (1025, T) linear
    magnitude spectrogram ``decibel_to_magnitude(inv_normalize_decibel(spec.T, mel_ref_db, mel_max_db))``
    (tacotron/inference.py:93-101; computed on the host from the downloaded network output with the conversions of
    ``audio.conversion``) -- and ``waveforms`` the Griffin-Lim reconstructions the reference's ``__main__`` makes of them
    (:170-188).  ``settings``: ``momentum`` and ``phase_init`` as in ``synthesize_stream``, and no other."""
    loader = dataset_params.dataset_loader
    ref_db, max_db = np.float32(loader.mel_mag_ref_db), np.float32(loader.mel_mag_max_db)
    rng_db = np.float32(abs(float(ref_db)) + abs(float(max_db)))
    for parts in synthesize_stream.parts(model, batches, n_steps, n_iter, seed, copy=True, want_linear=True, **settings):
        lin = parts['linear']
        specs = []
        for b in range(lin.shape[0]):
            # inv_normalize_decibel, decibel_to_magnitude (reference audio/conversion.py:81-102, 32-53) in host arithmetic:
            # the device versions of audio.conversion would synchronise the stream that the next batch is running on
            db = (np.clip(lin[b].T, np.float32(0), np.float32(1)) - np.float32(1)) * rng_db + ref_db
            assert not (db < -100.0).any(), 'decibel_to_magnitude: values below -100 dB'
            specs.append(np.power(np.float32(10), db / np.float32(20)).astype(np.float32))
        yield dict(specs=specs, wavs=parts['wavs'])


def target_dir(out_dir):
    """the folder the files go to -- ``inference_params.synthesis_dir`` unless given --, which has to exist (reference
    tacotron/inference.py:131-133)"""
    out_dir = out_dir or inference_params.synthesis_dir
    if not os.path.isdir(out_dir):
        raise NotADirectoryError('The specified synthesis target folder does not exist.')
    return out_dir


def open_model(weights, dataset, device_id):
    """``(dataset, model)``: the LJSpeech helper where no dataset is given, and the model with ``weights`` restored"""
    from ..datasets.lj_speech import LJSpeechDatasetHelper
    dataset = dataset or LJSpeechDatasetHelper(dataset_folder=dataset_params.dataset_folder,
                                                char_dict=dataset_params.vocabulary_dict, fill_dict=False)
    return dataset, Tacotron(inputs=Tacotron.model_placeholders(), mode=Mode.PREDICT, weights=weights, device_id=device_id)


def open_files(weights, dataset, out_dir, device_id):
    """what the file helpers do ahead of their synthesis: ``(out_dir, dataset, model)`` of ``target_dir`` and ``open_model``"""
    return (target_dir(out_dir),) + open_model(weights, dataset, device_id)


def write_files(out_dir, s, parts):
    """What the file helpers do behind it, with the ``parts`` of the synthesis: ``{i+1}.marks.jsonl`` of the ``marks``,
    ``alignment_report.json`` of the ``records`` (every row with the index of its ``text`` where there is a ``piece_text``) and
    ``{i+1}.wav`` of the ``wavs``, in the format and at the rate of the ``output``; float32 files are peak-normalised on the way
    (``SynthSettings.file_norm``) unless they are empty.  Returns the helper's own parts: ``wavs`` as a list, ``report``, ``marks``."""
    written = dict(wavs=list(parts['wavs']))
    for i, m in enumerate(parts.get('marks', ())):
        marks_.write_marks(os.path.join(out_dir, '{}.marks.jsonl'.format(i + 1)), m)
    if 'records' in parts:
        written['report'] = attention_check.report(parts['records'])
        for row, t in zip(written['report'], parts.get('piece_text', ())):
            row['text'] = int(t)
        with open(os.path.join(out_dir, REPORT_FILE), 'w') as f:
            json.dump(written['report'], f, indent=1)
    for i, wav in enumerate(written['wavs']):
        save_wav(os.path.join(out_dir, '{}.wav'.format(i + 1)), wav, output_rate(model_params, s.output),
                 s.file_norm()[1] and len(wav) > 0, encoding=output_encoding(s.output))
    if 'marks' in parts:
        written['marks'] = parts['marks']
    return written


@takes_settings()
def synthesize_sentences(raw_sentences, weights, dataset=None, out_dir=None, device_id=0, seed=0, **settings):
    """The reference's ``__main__`` (tacotron/inference.py:130-200) as a function.

    raw text lines -> process_sentences -> pad -> model -> wavs -> ``{i+1}.wav`` (peak-normalised
    float32 WAV, save_wav(norm=True)).  Returns the list of waveforms.  With ``stop_at_silence_db`` every file ends
    ``silence_keep_ms`` behind its utterance's last frame above that threshold instead of after max_iterations frames.
    ``settings``: the keywords of ``SynthSettings`` (a ``speaking_rate`` of 1.2: a fifth faster; a
    ``pitch`` of 4 / 12: four semitones up).  With a ``loudness`` or a ``limiter`` the files hold the waveforms as the device left
    them, not peak-normalised.  With ``check_alignment`` the result is ``(waveforms, report)`` with ``report`` the list of ``{index,
    verdict, record}`` of ``attention_check.report``, also written to ``alignment_report.json`` beside the wavs.  With an
    ``output`` the files and the returned arrays are in that format and at that rate (16-bit or 8-bit PCM, G.711), peak-normalised
    on the device ahead of the encoder where the float files would have been on the way to the disk.  With ``marks`` the result
    gains, as its last element, the timing marks of every sentence with offsets into the RAW sentence, also written as
    ``{i+1}.marks.jsonl`` beside every wav (``marks.write_marks``); a sentence the front end cannot be mapped back to raises
    ValueError (``marks.token_spans``)."""
    s = SynthSettings(model_params, **settings)   # (ValueError before anything is loaded)
    out_dir, dataset, model = open_files(weights, dataset, out_dir, device_id)
    mark_texts = [(raw,) + marks_.token_spans(dataset, raw) for raw in raw_sentences] if s.marks else None
    id_sequences, sequence_lengths = dataset.process_sentences(raw_sentences)
    max_length = max(sequence_lengths)
    sentences = np.array([pad_sentence(np.frombuffer(q, dtype=np.int32), max_length) for q in id_sequences], dtype=np.int32)
    return write_files(out_dir, s, synthesize_batch.parts(model, sentences, seed=seed, peak_normalize=s.file_norm()[0], mark_texts=mark_texts,
                                                          **settings))


def envelope_mode(markup_pitch, pitch_mode, timbre):
    """``(envelope, timbre_st)`` of ``synthesize_marked``'s three pitch arguments.  ValueError for a mode that is not one of
    ``prosody.PITCH_MODES``, for 'envelope' without ``markup_pitch``, and for a ``timbre`` that is not a finite number of semitones
    in [-12, 12] or is other than 0 outside the envelope mode (where nothing could apply it)."""
    if pitch_mode not in prosody.PITCH_MODES:
        raise ValueError('synthesize_marked: pitch_mode must be one of {}, got {!r}'.format(prosody.PITCH_MODES, pitch_mode))
    envelope = pitch_mode == 'envelope'
    if envelope and not markup_pitch:
        raise ValueError("synthesize_marked: pitch_mode='envelope' needs markup_pitch=True")
    try:
        st = float(timbre)
    except (TypeError, ValueError):
        st = float('nan')
    if not -12.0 <= st <= 12.0:
        raise ValueError('synthesize_marked: timbre must be a finite number of semitones in [-12, 12], got {!r}'.format(timbre))
    if st != 0.0 and not envelope:
        raise ValueError("synthesize_marked: a timbre other than 0 needs pitch_mode='envelope', got {!r}".format(timbre))
    return envelope, st


def marked_settings(hp, settings, envelope=False):
    """the record of ``synthesize_marked``, for itself and for its file form: no pitch, unless the pitch is made on the envelope's
    side (``envelope``), where a global pitch adds to every token's"""
    s = SynthSettings(hp, **settings)
    if s.octaves != 0.0 and not envelope:
        raise ValueError('synthesize_marked: a pitch other than 0 is not supported with markup (the resampler is global), got {!r}'.format(
            settings.get('pitch') if settings.get('pitch_semitones') is None else settings['pitch_semitones']))
    return s


@takes_settings('check_alignment')
def synthesize_marked(model, marked_sentences, dataset, n_steps=None, n_iter=None, seed=0, peak_normalize=False, want_plan=False,
                      markup_pitch=False, pitch_mode='resample', timbre=0.0, **settings):
    """Sentences with prosody markup (``tacotron.prosody``: ``<prosody rate=.. volume=..>``, ``<emphasis>``, ``<break/>`` under an
    optional ``<speak>``) -> a list of B waveforms, row b cut to its own hop (n_out[b] - 1) samples (no reference counterpart).

    A composition of the engine's stages, in this order: ``encoder_forward``, ``decoder_forward`` with alignments,
    ``token_times`` (at most ``marks_max_jump`` tokens a step), ``postnet_forward``, with ``stop_at_silence_db`` ``speech_frames``
    on the normalised linear spectrogram; ONE download -- ``start`` and, with stopping on, the lengths: the path's one host wait --;
    the planner (``prosody.token_attributes`` and ``prosody.segments_of_row``: every token's frames at its span's rate and gain,
    every break a pause, borders at decoder steps); ``denorm_power``, ``warp_magnitudes``, the ragged Griffin-Lim on ``n_out``, a
    peak normalisation per row (``peak_normalize``) or the ``loudness``, the ``limiter``, and ``deliver_rows`` for an
    ``output``.  The settings: as ``SynthSettings`` has them; ``speaking_rate`` is the base rate every span's rate multiplies.  A
    ``pitch`` other than 0 is a ValueError: the global resampler lives inside tts_synthesize; a pitch per word comes from the
    markup itself, with ``markup_pitch`` (below).  Sentences without markup at rate 1.0 give the bits of the same stages without the
    warp.

    With ``marks`` the result gains the timing marks of every sentence (``marks.marks_of_row`` at rate 1.0 through
    ``prosody.warp_position``: a slowed word's mark grows with it, a break opens a gap between two words' marks; ``start`` and
    ``end`` of a mark are offsets into the sentence with the markup removed); with ``want_plan`` a last element ``dict(plain,
    start, n_sent, n_frames, segments, n_out)``: what the call planned from, per row.

    ``markup_pitch``: ``<prosody pitch=..>`` is accepted (``prosody.parse_markup(.., pitch=True)``).  A word ``st`` semitones up
    is stretched by a further 2 ** (-st / 12) in the warp, and between Griffin-Lim and the finishing tail ``resample_segments``
    (tts_resample_segments) takes its samples back by that ratio (``prosody.pitch_segments_of_row``): the word lasts as long as it
    would without the pitch, a row without a pitch inside such a call is one copy segment and keeps its bits, and the tail gets
    the retimed rows' lengths.  The marks then go through ``prosody.pitch_position(hop * prosody.warp_position(..))``, and the
    plan gains ``pitch_segments`` and ``n_samples``, per row (None and hop (n_out - 1) where no pass ran).  If no sentence of the
    call holds a pitch other than 0 the pass is not launched: the bits of the call without the option.  More than
    ``RESAMPLE_SEGMENTS_MAX_RATIOS`` distinct ratios below 1 (pitches above 0) in one call is a ValueError that gives the count;
    the global ``pitch`` stays refused.

    ``pitch_mode`` 'envelope' (with ``markup_pitch``; the default 'resample' is the above): the pitch is made ahead of Griffin-Lim on
    the frequency axis and the formants stay where they are.  ``shift_magnitudes`` (tts_shift_magnitudes) runs between
    ``denorm_power`` and ``warp_magnitudes`` on the frames of every speech segment (``prosody.shift_segments_of_row``), nothing is
    stretched further and no ``resample_segments`` runs: the warp's segments are planned from the attributes without the pitch, so the
    row lengths and the marks are exactly those of the same text without any pitch (``prosody.warp_position`` alone).  Here the global ``pitch`` (octaves) is accepted and adds to every token's, and
    ``timbre`` (semitones in [-12, 12]) moves the envelope of every frame; the sum of a token's pitches must stay within an
    octave.  The plan gains ``shift_segments``, per row (None where the stage did not run).  If the text holds no pitch and both
    ``pitch`` and ``timbre`` are 0 the stage is not launched: the bits of the call without the option.  The order of the envelope
    is ``shift_order`` of the model's sampling rate; it, the lifter and the folding are untuned."""
    envelope, timbre_st = envelope_mode(markup_pitch, pitch_mode, timbre)
    s = marked_settings(model, settings, envelope)
    hp = model.hparams
    c = call_constants(model, n_steps, n_iter)
    hop, r = c.hop, hp.reduction
    parsed = [prosody.parse_markup(text, pitch=bool(markup_pitch)) for text in marked_sentences]
    if not parsed:
        raise ValueError('synthesize_marked: no sentence')
    plains = [p[0] for p in parsed]
    texts = [marks_.token_spans(dataset, plain) for plain in plains]
    planned = [prosody.token_attributes(dataset, plain, spans, breaks, s.rate, hop, hp.sampling_rate, pitch=bool(markup_pitch), pitch_mode=pitch_mode)
               for plain, spans, breaks in parsed]
    pitched = bool(markup_pitch) and not envelope and any(a[2] != 1.0 for attrs, _breaks in planned for a in attrs)
    # the envelope's side: every token's semitones with the global pitch added; the stage runs where any step is not 65536
    global_st = 12.0 * s.octaves if envelope else 0.0
    shifted = envelope and (timbre_st != 0.0 or any(shift_step(a[2] + global_st) != 65536 for attrs, _breaks in planned for a in attrs))
    below = {a[2] for attrs, _breaks in planned for a in attrs if a[2] < 1.0} if pitched else ()
    if len(below) > RESAMPLE_SEGMENTS_MAX_RATIOS:
        raise ValueError('synthesize_marked: {} distinct pitches above 0 in one call are more than the {} ratios below 1 that '
                         'resample_segments takes'.format(len(below), RESAMPLE_SEGMENTS_MAX_RATIOS))
    id_sequences, n_sent = dataset.process_sentences(plains)
    rows = [np.frombuffer(q, dtype=np.int32) for q in id_sequences]
    for b, (processed, _spans) in enumerate(texts):
        if int(n_sent[b]) != len(processed) + 1:
            raise ValueError('synthesize_marked: sentence {} has {} tokens, {} characters and the end token were expected'.format(
                b + 1, int(n_sent[b]), len(processed)))
    ids = np.array([pad_sentence(q, max(n_sent)) for q in rows], dtype=np.int32)
    n_sent = np.asarray(n_sent, dtype=np.int32)
    B, T = ids.shape[0], c.T
    eng = model.engine
    min_frames = (hp.n_fft // 2) // hop + 2      # Griffin-Lim's least: hop (n - 1) > n_fft / 2
    finish = finishing_tail('synthesize_marked', s, eng.sampling_rate)
    memory = eng.encoder_forward(ids)
    mel, alignments = eng.decoder_forward(memory, c.S)
    d_start, d_stats = eng.token_times(alignments, n_sent=n_sent, max_jump=s.marks_max_jump, to_host=False)
    mel.shape = (B, T, hp.n_mels)
    linear = eng.postnet_forward(mel)
    d_frames = d_last = None
    if s.stop is not None:
        threshold = eng.speech_threshold(s.stop[0], c.ref_db, c.max_db)
        d_frames, d_last = eng.speech_frames(linear, threshold, s.stop[1], min_frames)
    start = d_start.to_host()                    # (the one host wait)
    stats = d_stats.to_host()
    n_frames = d_frames.to_host().astype(np.int32) if d_frames is not None else np.full(B, T, dtype=np.int32)
    for a in (d_start, d_stats, d_frames, d_last, memory, alignments):
        if a is not None:
            a.free()
    segments, n_out, per_row, per_row_pitch, per_row_shift = [], [], [], [], []
    for b in range(B):
        seg, n, *ratios = prosody.segments_of_row(start[b], int(n_sent[b]), r, int(n_frames[b]), planned[b][0], planned[b][1], min_frames, row=b)
        if pitched:
            per_row_pitch.append(prosody.pitch_segments_of_row(seg, ratios[0], hop, n, row=b)[0])
        if envelope:
            # the warp's segments are those of the text without any pitch -- a border between two pitches alone must not cut a segment, or
            # the frame it rounds up to would move --; the cut at the pitches serves the shift alone
            if shifted:
                per_row_shift.append(prosody.shift_segments_of_row(seg, [0.0 if q[2] == 0 else st + global_st for q, st in zip(seg, ratios[0])],
                                                                   timbre_st, row=b))
            seg, n = prosody.segments_of_row(start[b], int(n_sent[b]), r, int(n_frames[b]), [a[:2] for a in planned[b][0]], planned[b][1],
                                             min_frames, row=b)
        per_row.append(seg)
        segments += seg
        n_out.append(n)
    mag = eng.denorm_power(linear, c.ref_db, c.max_db, hp.magnitude_power)
    plain_mag = None
    if shifted:
        plain_mag, mag = mag, eng.shift_magnitudes(mag, [q for seg in per_row_shift for q in seg], n_frames)
    warped, _n = eng.warp_magnitudes(mag, segments, n_frames)
    assert _n.tolist() == n_out, (_n, n_out)
    wav, _mse = eng.griffin_lim(warped, c.n_iter, c.win_len, hop, hp.n_fft, seed=seed, want_mse=False, momentum=s.momentum, n_frames=n_out,
                                phase_init=s.phase_init)
    held = hop * (np.asarray(n_out, dtype=np.int32) - 1)
    retimed = None
    if pitched:
        retimed, n_samples = eng.resample_segments(wav, [q for seg in per_row_pitch for q in seg], held)
        held = n_samples.astype(np.int32)
    wavs = finish(eng, wav if retimed is None else retimed, held, seed, peak_normalize)
    for a in (mel, linear, plain_mag, mag, warped, wav, retimed):
        if a is not None:
            a.free()
    parts = dict(wavs=wavs)
    if s.marks:
        all_marks = []
        for b, (processed, spans) in enumerate(texts):
            place = lambda x, seg=per_row[b]: float(hop) * prosody.warp_position(seg, x / float(hop), 'right')
            place_end = lambda x, seg=per_row[b]: float(hop) * prosody.warp_position(seg, x / float(hop), 'left')
            if pitched:
                place = lambda x, seg=per_row_pitch[b], warped_at=place: prosody.pitch_position(seg, warped_at(x), 'right')
                place_end = lambda x, seg=per_row_pitch[b], warped_at=place_end: prosody.pitch_position(seg, warped_at(x), 'left')
            all_marks.append(marks_.marks_of_row(processed, spans, start[b], r, hop, 1.0, hop * (int(n_frames[b]) - 1), hp.sampling_rate,
                                                 output_rate(hp, s.output), len(wavs[b]), s.marks, raw=plains[b], stats=stats[b],
                                                 place=place, place_end=place_end))
        parts['marks'] = all_marks
    if want_plan:
        parts['plan'] = dict(plain=plains, start=start, n_sent=n_sent, n_frames=n_frames, segments=per_row, n_out=n_out)
        if markup_pitch:
            parts['plan'].update(pitch_segments=per_row_pitch if pitched else None, n_samples=[int(v) for v in held])
        if envelope:
            parts['plan'].update(shift_segments=per_row_shift if shifted else None)
    return parts


@takes_settings('check_alignment')
def synthesize_marked_sentences(raw_sentences, weights, dataset=None, out_dir=None, device_id=0, seed=0, markup_pitch=False, pitch_mode='resample',
                                timbre=0.0, **settings):
    """``synthesize_sentences`` for sentences with prosody markup (``synthesize_marked``; ``settings``: its settings): ``{i+1}.wav`` per
    sentence -- peak-normalised unless a ``loudness`` or a ``limiter`` is set -- and, with ``marks``, ``{i+1}.marks.jsonl`` beside it
    with offsets into the sentence with the markup removed.  Returns the list of waveforms, with ``marks`` ``(waveforms, marks)``.
    ``markup_pitch``, ``pitch_mode`` and ``timbre``: as in ``synthesize_marked``."""
    envelope, _st = envelope_mode(markup_pitch, pitch_mode, timbre)
    s = marked_settings(model_params, settings, envelope)   # (ValueError before anything is loaded)
    for text in raw_sentences:
        prosody.parse_markup(text, pitch=bool(markup_pitch))
    out_dir, dataset, model = open_files(weights, dataset, out_dir, device_id)
    return write_files(out_dir, s, synthesize_marked.parts(model, raw_sentences, dataset, seed=seed, peak_normalize=s.file_norm()[0],
                                                           markup_pitch=markup_pitch, pitch_mode=pitch_mode, timbre=timbre, **settings))


# The pause behind a piece by the break that ends it, in milliseconds.  Untuned: round figures in the range speech synthesizers
# commonly use, not measured against recordings.
PAUSES_MS = {'paragraph': 700.0, 'sentence': 350.0, 'clause': 120.0, 'word': 0.0, 'cut': 0.0}
FADE_MS = 5.0               # the edge fades of a piece (110 samples at 22 050 Hz): untuned
LIMITED_MAX_PEAK = 4.0      # --loudness with --limit and no --max-peak: +12 dB of headroom for the limiter to take back; untuned
STOP_AT_SILENCE_DB = -40.0  # where synthesize_text ends a piece unless the caller says otherwise


def pause_samples(pauses_ms, sampling_rate):
    """``pauses_ms`` -- None or a dict {break: milliseconds} that overrides PAUSES_MS where it has a key -- as {break: samples}
    for all five breaks (ms_to_samples).  ValueError for a key that is no break or a pause that is not a finite number >= 0."""
    pauses = dict(PAUSES_MS)
    if pauses_ms is not None:
        if not isinstance(pauses_ms, dict):
            raise ValueError('pauses_ms must be None or a dict of {{break: ms}} with breaks among {}, got {!r}'.format(BREAKS, pauses_ms))
        for kind, ms in pauses_ms.items():
            if kind not in BREAKS:
                raise ValueError('pauses_ms: {!r} is not one of {}'.format(kind, BREAKS))
            try:
                ok = 0.0 <= float(ms) < float('inf')
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError('pauses_ms[{!r}] must be a finite number of milliseconds >= 0, got {!r}'.format(kind, ms))
            pauses[kind] = float(ms)
    out = {kind: ms_to_samples(ms, sampling_rate) for kind, ms in pauses.items()}
    if max(out.values()) >= 2 ** 31:
        raise ValueError('pauses_ms: a pause of {} samples does not fit the join'.format(max(out.values())))
    return out


def fade_samples(fade_ms, sampling_rate):
    """``fade_ms`` as the ``fade`` of ``Engine.join`` in samples (ms_to_samples).  ValueError for a fade that is not a finite number
    >= 0 or is longer than the join takes (tts_join_max_fade)."""
    try:
        ok = 0.0 <= float(fade_ms) < float('inf')
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('fade_ms must be a finite number of milliseconds >= 0, got {!r}'.format(fade_ms))
    fade = ms_to_samples(float(fade_ms), sampling_rate)
    if fade > JOIN_MAX_FADE:
        raise ValueError('fade_ms = {!r} is {} samples, more than the join takes ({})'.format(fade_ms, fade, JOIN_MAX_FADE))
    return fade


def lead_frames(first_active, speaking_rate, keep_frames):
    """the frames of a piece's waveform in front of its speech that the join leaves out: max(0, floor(max(0, first_active - 1) /
    speaking_rate) - keep_frames) -- the first active frame of the network's spectrogram, one frame of margin, taken to the
    stretched time axis, less the frames kept around speech"""
    return max(0, int(np.floor(max(0, int(first_active) - 1) / float(speaking_rate))) - int(keep_frames))


def pack_pieces(texts, dataset, batch_size, max_chars):
    """Every text split (``split_text`` with the dataset's abbreviations) and the pieces packed in order into calls of at most
    ``batch_size`` rows: ``(calls, piece_text, piece_break, pieces)`` with ``calls`` a list of ``(first piece, ids (B, T_sent)
    int32)``, each padded to its own longest row, and per piece its text's index, the break behind it and its characters."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError('batch_size must be an integer >= 1, got {!r}'.format(batch_size))
    if isinstance(texts, str):
        raise ValueError('texts must be a list of strings, not one string')
    piece_text, piece_break, pieces = [], [], []
    abbreviations = abbreviations_of(dataset)
    for t, text in enumerate(texts):
        for piece, brk in split_text(text, max_chars, abbreviations):
            piece_text.append(t)
            piece_break.append(brk)
            pieces.append(piece)
    calls = []
    if pieces:
        id_sequences, sequence_lengths = dataset.process_sentences(pieces)
        rows = [np.frombuffer(q, dtype=np.int32) for q in id_sequences]
        for p0 in range(0, len(rows), int(batch_size)):
            chunk = rows[p0:p0 + int(batch_size)]
            longest = max(len(r) for r in chunk)
            calls.append((p0, np.array([pad_sentence(r, longest) for r in chunk], dtype=np.int32)))
    return calls, piece_text, piece_break, pieces


def join_list_of_call(piece_text, piece_break, n_frames, first_active, hop, pauses, speaking_rate, keep_frames, lead_trim):
    """The edit list of one call: per row its text, the break behind it, the call's frame counts and first active frames ->
    ``(pieces (P, 4), groups (P,), texts, tail, orphans)``: the kept rows as ``row, first, count, gap`` with first = hop * lead and
    count = hop * (n_frames - 1) - first, one group per text that keeps a piece (``texts``: their indices, ascending), and ``tail``:
    per such text the pause behind its last kept piece.  A row without an active frame (or with nothing left behind its lead) is
    dropped and its pause kept: it goes to the kept piece in front of it in the same text and call, and where the call has none to
    ``orphans``, a list of ``(text, pause)`` in the order of the rows -- the caller adds those to the pause behind the part of the
    text that an earlier call said."""
    pieces, groups, texts, tail, orphans = [], [], [], [], []
    for b, t in enumerate(piece_text):
        gap = pauses[piece_break[b]]
        lead = lead_frames(first_active[b], speaking_rate, keep_frames) if lead_trim and first_active[b] >= 0 else 0
        first = hop * lead
        count = hop * (int(n_frames[b]) - 1) - first
        if first_active[b] < 0 or count < 1:
            if texts and texts[-1] == t:
                pieces[-1][3] += gap
                tail[-1] += gap
            else:
                orphans.append((t, gap))
            continue
        if not texts or texts[-1] != t:
            texts.append(t)
            tail.append(0)
        pieces.append([b, first, count, gap])
        groups.append(len(texts) - 1)
        tail[-1] = gap
    return np.array(pieces, dtype=np.int64).reshape(-1, 4), np.array(groups, dtype=np.int64), texts, tail, orphans


def text_plan(caller, hp, pauses_ms, fade_ms, settings):
    """What ``synthesize_text`` checks ahead of everything else, for itself and for its file form: ``(record, pauses, fade)`` --
    the ``settings`` with ``stop_at_silence_db`` at -40 dB unless given, which cannot be None; ``pause_samples``; ``fade_samples``."""
    s = SynthSettings(hp, **dict({'stop_at_silence_db': STOP_AT_SILENCE_DB}, **settings))
    if s.stop is None:
        raise ValueError('{}: stop_at_silence_db cannot be None (pieces of max_iterations frames cannot be joined)'.format(caller))
    rate = getattr(hp, 'hparams', hp).sampling_rate
    return s, pause_samples(pauses_ms, rate), fade_samples(fade_ms, rate)


@takes_settings()
def synthesize_text(model, texts, dataset, batch_size=64, pauses_ms=None, fade_ms=FADE_MS, lead_trim=True, max_chars=MAX_CHARS,
                    n_steps=None, n_iter=None, seed=0, peak_normalize=False, **settings):
    """Texts of any length -> one float32 waveform per text (no reference counterpart: tacotron/inference.py:139-200 makes one
    file of at most max_iterations frames per line).

    Every text is split into pieces of at most ``max_chars`` characters (``datasets.text_split.split_text`` with the dataset's
    abbreviations), the pieces become ids (``process_sentences``, ``pad_sentence``) and are packed in order into calls of at most
    ``batch_size`` rows (``pack_pieces``); call k runs ``Engine.synthesize`` with seed ``seed`` + k, no normalisation, and leaves
    its waveforms on the device.  ``settings``: the keywords of ``SynthSettings``; ``stop_at_silence_db`` defaults to -40 dB here and
    cannot be None, because a piece that runs on to max_iterations frames is of no use in a joined text.

    Piece b of a call is cut from its row as ``first = hop * lead`` and ``count = hop * (n_frames[b] - 1) - first``, with lead =
    ``lead_frames(first_active[b], speaking_rate, keep_frames)`` -- ``first_active`` from ``Engine.speech_interval`` on the call's
    normalised linear spectrogram at the stopping threshold -- or 0 with ``lead_trim`` off.  A piece without an active frame is
    dropped and its pause added to the one in front of it -- the pause of the piece before it, or of the part of its text that an
    earlier call said; in front of a text's first spoken sample nothing is kept.  The pause behind a piece follows its break (``pauses_ms`` over
    PAUSES_MS: paragraph 700, sentence 350, clause 120, word and cut 0 ms -- untuned), every piece fades over ``fade_ms`` at
    either edge, and one ``Engine.join`` per call lays the pieces of each text into one row on the device.  With a ``loudness``
    one ``Engine.loudness_normalize`` runs over the joined rows, so a text is levelled as a whole and its sentences keep their
    relative levels; with a ``limiter`` one ``Engine.limit`` runs over the joined rows behind it, and with an ``equalizer`` one
    ``Engine.equalize`` and with a ``compressor`` one ``Engine.compress`` ahead of both, in that order: a text is compressed as a
    whole, after the join; with a ``watermark`` one ``Engine.watermark_embed`` behind the compressor, so the carrier starts at the
    file's first sample.  Only the n_out[g] samples of a row that were said are downloaded.

    A text whose pieces span several calls is concatenated on the host, with the pause behind the earlier part as zeros between
    them; with a ``loudness`` each part is levelled on its own.  The packing decides which pieces share a call, a call's seed
    and the length its ids are padded to, so the bits of a text may depend on ``batch_size`` and on the texts around it.

    With an ``output`` the JOINED texts, not the pieces, are resampled and encoded (``deliver``: one batch of all the texts, the
    dither's seed ``seed``, text t dithered as row t of the texts that say something), behind a peak normalisation of each whole
    text with ``peak_normalize``; the waveforms are then that format's codes at its rate.

    Returns the list of waveforms (a text without a piece that speaks: an empty array); with ``check_alignment`` ``(waveforms,
    records, verdicts, piece_text)``: the alignment record and ``attention_check.verdict`` of every piece, in order, and the
    index of the text each piece belongs to.  With ``marks`` ('word' or 'char') the result gains, as its last element, the timing
    marks of every text in ITS waveform (``marks.marks_of_text``): every piece's marks taken through its lead trim, the join's
    layout and the parts of a text that span calls, with offsets into the raw text; a dropped piece's marks have no length."""
    s, pauses, fade = text_plan('synthesize_text', model, pauses_ms, fade_ms, settings)
    hp = model.hparams
    calls, piece_text, piece_break, _pieces = pack_pieces(texts, dataset, batch_size, max_chars)
    piece_at = []                   # with marks: per piece its (processed, spans) in its raw text, in the order of pack_pieces
    if s.marks:
        for text in texts:
            piece_at += [marks_.piece_spans(dataset, text, a, b) for _p, _k, a, b in split_text_spans(text, max_chars, abbreviations_of(dataset))]
    marked = [[] for _ in texts]    # ... and per text what marks_of_text takes of its pieces
    c = call_constants(model, n_steps, n_iter)
    win_hop = c.hop
    eng = model.engine
    finish = finishing_tail('synthesize_text', s, eng.sampling_rate, deliver=False)   # (the output is made of the whole texts, below)
    keep_frames = s.stop[1]
    threshold = eng.speech_threshold(s.stop[0], c.ref_db, c.max_db)
    parts = [[] for _ in texts]     # per text the waveforms of its parts, one per call that says some of it
    tails = [0 for _ in texts]      # ... and the pause behind the last part so far
    records = []
    for k, (p0, ids) in enumerate(calls):
        B = ids.shape[0]
        out = eng.synthesize(ids, *c.synth, seed=seed + k, peak_normalize=False, want_linear=True,
                             **dict(s.engine_keywords(), loudness=None, limiter=None, equalizer=None, compressor=None, watermark=None))   # (all five run on the joined rows)
        first_active = eng.speech_interval(out['linear'], threshold)[0].to_host()
        if s.check_alignment:
            records.append(eng.synth_alignment_stats(B))
        pieces, groups, said, tail, orphans = join_list_of_call(piece_text[p0:p0 + B], piece_break[p0:p0 + B], out['n_frames'], first_active,
                                                                win_hop, pauses, s.rate, keep_frames, lead_trim)
        for t, gap in orphans:      # (silent pieces in front of the call's first kept piece of their text)
            if parts[t]:
                tails[t] += gap
        if s.marks:
            start, tstats = eng.synth_token_times(B)
            o, kept = marks_.join_offsets(pieces, groups), {int(row[0]): i for i, row in enumerate(pieces)}
            for b in range(B):
                t = piece_text[p0 + b]
                so_far = sum(len(w) for w in parts[t])
                entry = dict(processed=piece_at[p0 + b][0], spans=piece_at[p0 + b][1], start=start[b], stats=tstats[b])
                if b in kept:
                    i = kept[b]
                    entry.update(n_held=win_hop * (int(out['n_frames'][b]) - 1), first=int(pieces[i][1]), count=int(pieces[i][2]), o=int(o[i]),
                                 part=so_far + tails[t] if parts[t] else 0, end=0)
                    entry['end'] = entry['o'] + entry['count'] + entry['part']
                else:               # dropped: at the end of what its text has said so far
                    before = [e for e in marked[t] if 'end' in e and e.get('call') == k]
                    entry['at'] = before[-1]['end'] if before else so_far
                entry['call'] = k
                marked[t].append(entry)
        if not said:
            continue
        joined, n_out = eng.join(out['wav'], pieces, groups, fade)
        for t, wav, gap in zip(said, finish(eng, joined, n_out), tail):
            if parts[t]:
                parts[t].append(np.zeros(tails[t], dtype=np.float32))
            parts[t].append(wav)
            tails[t] = gap
    wavs = [np.concatenate(p) if p else np.zeros(0, dtype=np.float32) for p in parts]
    if s.output is not None:
        wavs = deliver(eng, wavs, s.output, seed, norm=peak_normalize, what='text')
    elif peak_normalize:
        raise ValueError('synthesize_text: peak_normalize goes with an output (save_wav normalises float32 files)')
    named = dict(wavs=wavs)
    if s.check_alignment:
        named['records'] = np.concatenate(records) if records else np.zeros(0, dtype=ALIGNMENT_RECORD)
        named['verdicts'], named['piece_text'] = attention_check.verdict(named['records']), list(piece_text)
    if s.marks:
        named['marks'] = [marks_.marks_of_text(marked[t], hp.reduction, win_hop, s.rate, hp.sampling_rate, output_rate(model, s.output),
                                               len(wavs[t]), s.marks, raw=texts[t]) for t in range(len(texts))]
    return named


@takes_settings()
def synthesize_texts(raw_texts, weights, dataset=None, out_dir=None, device_id=0, seed=0, batch_size=64, pauses_ms=None,
                     fade_ms=FADE_MS, lead_trim=True, max_chars=MAX_CHARS, **settings):
    """``synthesize_sentences`` for texts of any length: every entry of ``raw_texts`` becomes one ``{i+1}.wav`` that holds the whole
    text (``synthesize_text``, with its keywords).  Without a ``loudness`` or a ``limiter`` each file is peak-normalised once by save_wav,
    as the sentence files are; a text that says nothing gives an empty file.  Returns the list of waveforms, with ``check_alignment``
    ``(waveforms, report)`` -- one ``{index, verdict, record}`` per PIECE, each with the index of its ``text`` -- also written to
    ``alignment_report.json``.  With ``marks`` the result gains the timing marks of every text as its last element, also written as
    ``{i+1}.marks.jsonl`` beside every wav."""
    target_dir(out_dir)
    s = text_plan('synthesize_texts', model_params, pauses_ms, fade_ms, settings)[0]   # (ValueError before anything is loaded)
    out_dir, dataset, model = open_files(weights, dataset, out_dir, device_id)
    return write_files(out_dir, s, synthesize_text.parts(model, raw_texts, dataset, batch_size, pauses_ms, fade_ms, lead_trim, max_chars,
                                                         seed=seed, peak_normalize=s.file_norm()[0], **settings))


def read_texts(path):
    """``read_sentences`` for ``--text``: every line is one text, and the two-character sequence backslash-n twice in a row marks
    a paragraph break inside it (a line cannot hold a newline)"""
    return [line.replace('\\n\\n', '\n\n') for line in read_sentences(path)]


def pause_option(option):
    """``KIND=MS`` of ``--pause-ms`` as ``(kind, ms)``"""
    import argparse
    kind, sep, ms = option.partition('=')
    try:
        if not sep or kind not in BREAKS:
            raise ValueError
        return kind, float(ms)
    except ValueError:
        raise argparse.ArgumentTypeError('KIND=MS with KIND one of {} is needed, got {!r}'.format(', '.join(BREAKS), option))


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
                                                            [--eq PROFILE|kind:f0[:q][:gain_db],...]
                                                            [--compress PROFILE|T:R[:knee[:attack[:release[:makeup]]]]]
                                                            [--watermark KEY[:PAYLOAD]]
                                                            [--limit DB [--limit-lookahead-ms MS] [--sample-peak]]
                                                            [--format pcm16|pcm8|mulaw|alaw|float32 [--out-rate HZ] [--no-dither]]
                                                            [--check-alignment] [--marks [word|char] [--marks-max-jump J]]
                                                            [--text [--max-chars N] [--pause-ms KIND=MS ...] [--fade-ms MS]]
                                                            [--markup [--markup-pitch [--pitch-mode resample|envelope] [--timbre ST]]]

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
    ``--eq``: an equaliser shapes the spectrum of every wav ahead of the loudness gain and the limiter: a profile -- ``telephony``
    (300 .. 3400 Hz, 4th-order Butterworth edges: what ``--format mulaw --out-rate 8000`` wants in front of it), ``small-speaker``,
    ``rumble``, ``bright``, ``warm``; every preset is untuned -- or up to 8 sections ``kind:f0[:q][:gain_db]`` separated by commas,
    kinds lowpass, highpass, peak, lowshelf, highshelf, e.g. ``--eq highpass:120,peak:3000:1.0:+3,highshelf:6000:+2``.  A boost can
    take samples beyond 1: give it ``--limit`` or ``--loudness``.
    ``--compress``: a feed-forward peak compressor lowers the crest factor of every wav behind the equaliser and ahead of the
    loudness gain and the limiter: a profile -- ``speech``, ``telephony``, ``small-speaker``; every preset is untuned -- or
    ``T:R[:knee[:attack[:release[:makeup]]]]``: the threshold in dB re full scale, the ratio (``inf`` allowed), the knee's width in
    dB (6), the attack and release in ms (5 and 100) and the make-up gain in dB (0), e.g. ``--compress=-18:3:6:5:100:3`` (with the equals sign: the value begins with a minus).  A make-up
    gain can take samples beyond 1: give it ``--limit`` or ``--loudness``.
    ``--watermark KEY[:PAYLOAD]``: a keyed spread-spectrum carrier is added under the local envelope of every wav, behind the
    compressor and ahead of the loudness gain and the limiter; ``python -m single-speaker-tts_amd.tacotron.detect --key KEY file.wav``
    finds it and reads the payload (16 bits) back.  KEY and PAYLOAD are integers, decimal or 0x-hexadecimal.  The carrier's shape and
    strength are the UNTUNED defaults: nobody has listened.
    ``--limit DB``: a look-ahead peak limiter runs last over every wav: no peak above DB decibels relative to full scale (e.g.
    -1), looking ``--limit-lookahead-ms`` ahead (default 5); the ceiling holds for the interpolated (true) peaks, with
    ``--sample-peak`` for the samples alone.  The files are then not peak-normalised.  With ``--loudness`` and no ``--max-peak``
    the loudness gain may then produce samples up to 4.0 (+12 dB of headroom, which the limiter takes back; untuned).
    ``--format``: the sample format of the files -- 16-bit PCM, unsigned 8-bit PCM, ITU-T G.711 mu-law or A-law, or the
    reference's float32 (default) -- at ``--out-rate`` Hz (default: the model's rate; within a factor of 4 of it), encoded on
    the device with TPDF dither unless ``--no-dither``; e.g. ``--format mulaw --out-rate 8000`` for telephony.  A file whose
    samples clipped in the encoder is reported with its count: with ``--limit -1`` there is head room for the resampler.
    ``--check-alignment``: the attention diagnostics (``tacotron.attention_check``) -- one JSON line per sentence (index,
    verdict, record) and ``alignment_report.json`` beside the wavs; the exit status stays 0 whatever the verdicts.
    ``--marks``: timing marks -- when every word (``--marks char``: and every character) is spoken, in milliseconds and in samples
    of the file, with offsets into the line -- as JSON lines in ``{i+1}.marks.jsonl`` beside every wav (``tacotron.marks``); the
    search lets a decoder step advance over at most ``--marks-max-jump`` characters (default 4, untuned).
    ``--text``: every line of the synthesis file is a text of any length -- sentences, paragraphs (the two characters ``\\n``
    twice in a row mark a paragraph break inside a line) -- and ``{i+1}.wav`` holds the whole text (``synthesize_text``): split
    into pieces of at most ``--max-chars`` characters (default 150), each stopped at its silence (``--stop-at-silence``, -40 dB
    unless given), joined on the device with the pause of its break (``--pause-ms sentence=350``, repeatable; paragraph,
    sentence, clause, word, cut) and edge fades of ``--fade-ms`` (default 5).  With ``--loudness`` a text is levelled as a whole.
    ``--markup``: every line of the synthesis file is a sentence with prosody markup (``tacotron.prosody``, a subset of SSML):
    ``<prosody rate="80%" volume="-6 dB">``, ``<emphasis level="strong">`` and ``<break time="300ms"/>`` change the rate, the volume
    and the pauses word by word (``synthesize_marked``; ``--rate`` is then the base rate).  Works with ``--marks``, whose offsets are
    then into the line with the markup removed; refused together with ``--text``, ``--pitch`` and ``--check-alignment``.
    ``--markup-pitch``: with ``--markup``, ``<prosody pitch="+2st">`` (or ``+N%``, x-low .. x-high; untuned presets) is accepted too
    and changes the pitch word by word, leaving every word's duration and the marks' meaning alone (``tts_resample_segments``).
    ``--pitch-mode envelope``: with ``--markup --markup-pitch``, the pitch is made on the frequency axis ahead of Griffin-Lim
    (``tts_shift_magnitudes``) and the formants stay where they are; ``--pitch`` is then allowed beside ``--markup`` and adds to every
    word, and ``--timbre ST`` moves the formants of every frame by ST semitones.  The default, ``resample``, is the above."""
    args = parse_args(argv)
    settings = settings_option(args)
    SynthSettings(model_params, **settings)
    # Before we start doing anything we check if the required target folder actually exists (:131-133)
    out_dir = target_dir(args.synthesis_dir)
    path = args.synthesis_file or inference_params.synthesis_file
    raw_sentences = read_texts(path) if args.text else read_sentences(path)
    print('{} {} were loaded for inference.'.format(len(raw_sentences), 'texts' if args.text else 'sentences'))
    if args.synthetic_weights is not None:
        from .weights import synthetic_weights
        weights = synthetic_weights(args.synthetic_weights, model_params)
    elif args.weights is not None:
        weights = args.weights
    elif inference_params.checkpoint_file is not None:
        weights = inference_params.checkpoint_file
    else:
        weights = os.path.join(inference_params.checkpoint_dir, inference_params.checkpoint_load_run)
    if args.markup:
        written = synthesize_marked_sentences.parts(raw_sentences, weights, None, out_dir, args.device, args.seed, markup_pitch=args.markup_pitch,
                                                    pitch_mode=args.pitch_mode, timbre=args.timbre, **settings)
    elif args.text:
        if args.stop_at_silence is None:
            settings['stop_at_silence_db'] = STOP_AT_SILENCE_DB
        written = synthesize_texts.parts(raw_sentences, weights, None, out_dir, args.device, args.seed, max_chars=args.max_chars,
                                          pauses_ms=dict(args.pause_ms), fade_ms=args.fade_ms, **settings)
    else:
        written = synthesize_sentences.parts(raw_sentences, weights, None, out_dir, args.device, args.seed, **settings)
    for row in written.get('report', ()):
        print(json.dumps(row))
    for i in range(len(written['wavs'])):
        print('Saved: "{}"'.format(os.path.join(out_dir, '{}.wav'.format(i + 1))))
    return 0


def settings_option(args):
    """the command line's options as the ``settings`` of the helpers above: the keywords of ``SynthSettings``"""
    return dict(momentum=args.momentum, stop_at_silence_db=args.stop_at_silence, silence_keep_ms=args.silence_keep_ms,
                speaking_rate=args.rate, pitch_semitones=args.pitch, phase_init=args.phase_init,
                loudness=None if args.loudness is None else (args.loudness, args.max_peak), check_alignment=args.check_alignment,
                limiter=None if args.limit is None else (10.0 ** (args.limit / 20.0), args.limit_lookahead_ms, 1 if args.sample_peak else 4),
                output=output_option(args), marks=args.marks, marks_max_jump=args.marks_max_jump, equalizer=eq_option(args.eq),
                compressor=compress_option(args.compress), watermark=watermark_option(args.watermark))


def watermark_option(text):
    """``--watermark`` as the ``watermark`` of the helpers above: None, or ``KEY[:PAYLOAD]`` as ``(key, payload)``, both integers,
    decimal or 0x-hexadecimal.  ValueError names the field."""
    if text is None:
        return None
    fields = text.split(':')
    if not 1 <= len(fields) <= 2:
        raise ValueError('--watermark: {!r}: KEY[:PAYLOAD] is needed'.format(text))
    try:
        values = tuple(int(v, 0) for v in fields)
    except ValueError:
        raise ValueError('--watermark: {!r}: the key and the payload must be integers (decimal or 0x...)'.format(text))
    return values + (0,) * (2 - len(values))


def compress_option(text):
    """``--compress`` as the ``compressor`` of the helpers above: None, a profile name, or ``T:R[:knee[:attack[:release[:makeup]]]]``
    as a tuple of numbers.  ValueError names the field."""
    if text is None or ':' not in text:
        return text
    fields = text.split(':')
    if not 2 <= len(fields) <= 6:
        raise ValueError('--compress: {!r}: T:R[:knee[:attack[:release[:makeup]]]] is needed'.format(text))
    try:
        return tuple(float(v) for v in fields)
    except ValueError:
        raise ValueError('--compress: {!r}: the fields must be numbers'.format(text))


def eq_option(text):
    """``--eq`` as the ``equalizer`` of the helpers above: None, a profile name, or ``kind:f0[:q][:gain_db]`` sections separated by
    commas -- a low-pass or high-pass takes ``kind:f0[:q]``, a peak or shelf with three fields ``kind:f0:gain_db`` (Q 0.7071...)
    and with four ``kind:f0:q:gain_db``.  ValueError names the field."""
    if text is None or ':' not in text:
        return text
    sections = []
    for part in text.split(','):
        kind, *fields = part.strip().split(':')
        try:
            numbers = [float(v) for v in fields]
        except ValueError:
            raise ValueError('--eq: {!r}: the fields behind the kind must be numbers'.format(part))
        gained = kind in ('peak', 'lowshelf', 'highshelf')
        if not 1 <= len(numbers) <= (3 if gained else 2):
            raise ValueError('--eq: {!r}: kind:f0[:q]{} is needed'.format(part, '[:gain_db]' if gained else ''))
        if gained and len(numbers) == 2:
            numbers = [numbers[0], None, numbers[1]]
        sections.append((kind,) + tuple(numbers))
    return sections


def output_option(args):
    """``--format`` / ``--out-rate`` / ``--no-dither`` as the ``output`` of the helpers above"""
    if args.format == 'float32' and args.out_rate is None:
        return None
    return (args.format, None if args.no_dither else 'tpdf', args.out_rate)


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
    ap.add_argument('--max-peak', type=float, default=argparse.SUPPRESS, metavar='P',
                    help='with --loudness: the largest |sample| the gain may produce (default {:g}; with --limit {:g})'.format(
                        LOUDNESS_MAX_PEAK, LIMITED_MAX_PEAK))
    ap.add_argument('--eq', default=None, metavar='PROFILE|SECTIONS',
                    help='an equaliser ahead of the loudness gain and the limiter: a profile (telephony, small-speaker, rumble, bright, warm; '
                         'untuned) or sections kind:f0[:q][:gain_db], e.g. highpass:120,peak:3000:1.0:+3,highshelf:6000:+2')
    ap.add_argument('--compress', default=None, metavar='PROFILE|T:R[:KNEE[:ATTACK[:RELEASE[:MAKEUP]]]]',
                    help='a peak compressor behind the equaliser, ahead of the loudness gain and the limiter: a profile (speech, telephony, '
                         'small-speaker; untuned) or threshold dB : ratio [: knee dB : attack ms : release ms : make-up dB], e.g. --compress=-18:3:6:5:100:3')
    ap.add_argument('--watermark', default=None, metavar='KEY[:PAYLOAD]',
                    help='a keyed carrier under the local envelope, behind the compressor and ahead of the loudness gain and the limiter '
                         '(untuned defaults); tacotron.detect --key KEY finds it, e.g. --watermark 0x5EED:0xA5C3')
    ap.add_argument('--limit', type=float, default=None, metavar='DB',
                    help='a look-ahead peak limiter behind everything else: no peak above DB decibels re full scale, e.g. -1')
    ap.add_argument('--limit-lookahead-ms', type=float, default=LIMIT_LOOKAHEAD_MS, metavar='MS',
                    help='with --limit: how far the limiter looks ahead (default {:g} ms)'.format(LIMIT_LOOKAHEAD_MS))
    ap.add_argument('--sample-peak', action='store_true', help='with --limit: hold the samples under the ceiling, not the interpolated peaks')
    ap.add_argument('--format', default='float32', choices=['float32', 'pcm16', 'pcm8', 'mulaw', 'alaw'],
                    help='the sample format of the wavs: float32 (default, the reference\'s), 16-bit or 8-bit PCM, G.711 mu-law or A-law')
    ap.add_argument('--out-rate', type=int, default=None, metavar='HZ',
                    help='the sampling rate of the wavs (default: the model\'s; within a factor of 4 of it), e.g. 8000 for telephony')
    ap.add_argument('--no-dither', action='store_true', help='with --format: round without the TPDF dither')
    ap.add_argument('--check-alignment', action='store_true',
                    help='attention diagnostics: one JSON line per sentence and {} beside the wavs'.format(REPORT_FILE))
    ap.add_argument('--marks', nargs='?', const='word', default=None, choices=list(marks_.KINDS),
                    help='timing marks of every word (or, with char, every character too) as JSON lines in {i+1}.marks.jsonl beside the wavs')
    ap.add_argument('--marks-max-jump', type=int, default=4, metavar='J',
                    help='with --marks: the most characters a decoder step may advance over, 1 .. 15 (default 4, untuned)')
    ap.add_argument('--text', action='store_true',
                    help='every line of the synthesis file is a text of any length (a literal \\n\\n marks a paragraph): one wav per text')
    ap.add_argument('--max-chars', type=int, default=MAX_CHARS, metavar='N',
                    help='with --text: the longest piece a text is cut into (default {}, the sentence length of the benchmark)'.format(MAX_CHARS))
    ap.add_argument('--pause-ms', type=pause_option, action='append', default=[], metavar='KIND=MS',
                    help='with --text: the pause behind a break, KIND one of {} (defaults {}; repeatable)'.format(
                        ', '.join(BREAKS), ', '.join('{}={:g}'.format(k, PAUSES_MS[k]) for k in BREAKS)))
    ap.add_argument('--fade-ms', type=float, default=FADE_MS, metavar='MS',
                    help='with --text: the fade at either edge of a piece (default {:g} ms)'.format(FADE_MS))
    ap.add_argument('--markup', action='store_true',
                    help='every line of the synthesis file is a sentence with prosody markup: <prosody rate= volume=>, <emphasis>, <break/> '
                         '(not with --text, --pitch or --check-alignment)')
    ap.add_argument('--markup-pitch', action='store_true',
                    help='with --markup: <prosody pitch=> is accepted too (+Nst, -Nst, +N%%, -N%%, x-low .. x-high): a pitch per word, at the '
                         'word\'s own duration')
    ap.add_argument('--pitch-mode', choices=prosody.PITCH_MODES, default='resample',
                    help='with --markup --markup-pitch: how a pitch is made -- resample (default): behind Griffin-Lim on the samples, the '
                         'formants move with the pitch; envelope: ahead of it on the frequency axis, the formants stay (--pitch is then allowed '
                         'and adds to every word)')
    ap.add_argument('--timbre', type=float, default=0.0, metavar='ST',
                    help='with --pitch-mode envelope: move the spectral envelope (the formants) of every frame by ST semitones, -12 .. 12 (untuned)')
    args = ap.parse_args(argv)
    if args.markup_pitch and not args.markup:
        ap.error('--markup-pitch requires --markup')
    envelope = args.pitch_mode == 'envelope'
    if envelope and not args.markup_pitch:
        ap.error('--pitch-mode envelope requires --markup --markup-pitch')
    if args.timbre != 0.0 and not envelope:
        ap.error('--timbre requires --pitch-mode envelope')
    if not -12.0 <= args.timbre <= 12.0:
        ap.error('--timbre must lie in [-12, 12] semitones')
    if args.markup and args.text:
        ap.error('--markup cannot be combined with --text (markup inside long texts is not supported)')
    if args.markup and args.pitch != 0.0 and not envelope:
        ap.error('--markup cannot be combined with --pitch (a pitch needs the call pipeline\'s resampler)')
    if args.markup and args.check_alignment:
        ap.error('--markup cannot be combined with --check-alignment')
    if not hasattr(args, 'max_peak'):
        args.max_peak = LIMITED_MAX_PEAK if args.limit is not None and args.loudness is not None else LOUDNESS_MAX_PEAK
    return args


if __name__ == '__main__':
    raise SystemExit(main())
