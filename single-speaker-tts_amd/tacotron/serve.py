"""Mirror of the reference's serving helpers (tacotron/serve.py:22-126) on the MI355X path.

``pre_process_sentences`` (:22-36) and ``post_process_spectrograms`` (:39-86) keep their names;
``serve`` (:89-126) is the same loop -- sentences from a generator, one batch per iteration --
driving the HIP library instead of a TensorFlow SavedModel session.  Unlike the reference's
``post_process_spectrograms`` (which squeezes a trailing axis and therefore only works for a batch
of one, serve.py:58), a whole batch is supported.
"""
import numpy as np

from .._hip import synth_frame_counts, synth_lengths
from . import attention_check, marks as marks_
from .inference import (SynthSettings, call_constants, deliver, finishing_tail, marks_of_batch, open_model, pad_id, pad_sentence,
                        synthesize_stream, takes_settings)
from .params import model_params


def pre_process_sentences(_sentences, dataset):
    """raw strings -> padded int32 id batch (reference tacotron/serve.py:22-36)."""
    id_sequences, sequence_lengths = dataset.process_sentences(_sentences)
    sentences = [np.frombuffer(s, dtype=np.int32) for s in id_sequences]
    max_length = max(sequence_lengths)
    return np.array([pad_sentence(s, max_length) for s in sentences], dtype=np.int32)


@takes_settings('check_alignment', 'output', 'marks', 'marks_max_jump')
def post_process_spectrograms(_spectrograms, engine, init_phase=None, seed=0, **settings):
    """normalised linear spectrograms (B, T, 1025) -> list of waveforms: de-normalise with the mel dB
    constants, ``** magnitude_power``, Griffin-Lim (reference tacotron/serve.py:39-86).  ``settings`` mean what
    ``inference.SynthSettings`` says -- the alignment check, the delivery format and the marks apart, which need more than
    spectrograms --, composed here from the engine's stages: with ``stop_at_silence_db``
    ``Engine.speech_frames`` on the normalised spectrograms, then one ragged Griffin-Lim call, every utterance returned at its own
    length; with a ``speaking_rate`` or a ``pitch`` ``Engine.stretch_magnitudes`` by rate * 2 ** -pitch ahead of Griffin-Lim
    (``init_phase`` has that many frames; lengths min(T', max(min_frames, ceil(n / rate)))) and ``Engine.resample`` by 2 ** -pitch
    behind it; with an ``equalizer`` ``Engine.equalize`` and with a ``compressor`` ``Engine.compress`` behind it, in that order;
    with a ``watermark`` ``Engine.watermark_embed`` behind those;
    with a ``loudness`` ``Engine.loudness_normalize``, every waveform measured over its own samples; with a ``limiter`` ``Engine.limit``
    last, over the same samples."""
    s = SynthSettings(model_params, **settings)
    stop, rate, octaves = s.stop, s.rate, s.octaves
    finish = finishing_tail('post_process_spectrograms', s, model_params.sampling_rate)
    rho = float(np.exp2(-np.float64(octaves)))
    c = call_constants(model_params)
    win_hop = c.hop
    spec = np.asarray(_spectrograms, dtype=np.float32)
    if spec.ndim == 2:
        spec = spec[None]
    n_frames = None
    T = spec.shape[1]
    min_frames = (model_params.n_fft // 2) // win_hop + 2   # the shortest signal Griffin-Lim takes: hop (n - 1) > n_fft / 2
    # the frames of the waveforms, with or without a pitch, and the frames Griffin-Lim reconstructs from (ValueError where
    # rate * rho leaves [0.25, 4])
    T_s, T_g = synth_frame_counts(T, rate, octaves)
    if rate != 1.0 and T_s < min_frames:
        raise ValueError('speaking_rate {}: {} frames are left of {}, at least {} needed'.format(rate, T_s, T, min_frames))
    if octaves != 0.0 and T_g < min_frames:
        raise ValueError('pitch {} at speaking_rate {}: {} frames are left of {}, at least {} needed'.format(octaves, rate, T_g, T, min_frames))
    if stop is not None:
        if T < min_frames:
            raise ValueError('stop_at_silence_db: spectrograms of {} frames, at least {} needed'.format(T, min_frames))
        thr = engine.speech_threshold(stop[0], c.ref_db, c.max_db)
        n_frames = engine.speech_frames(spec, thr, keep_frames=stop[1], min_frames=min_frames)[0].to_host()
    mag = engine.denorm_power(spec, c.ref_db, c.max_db, model_params.magnitude_power)
    n_gl = n_frames   # the frames Griffin-Lim runs on
    if rate != 1.0 or octaves != 0.0:
        mag = engine.stretch_magnitudes(mag, rate * rho, n_frames=n_frames, T_out=T_g)
        if n_frames is not None:
            n_frames, n_gl = synth_lengths(n_frames, T, rate, octaves, min_frames)
    wav, _ = engine.griffin_lim(mag, c.n_iter, c.win_len, win_hop, model_params.n_fft, init_phase=init_phase, seed=seed, want_mse=False,
                                momentum=s.momentum, n_frames=n_gl, phase_init=s.phase_init)
    if octaves != 0.0:
        gl_wav = wav
        try:
            wav = engine.resample(gl_wav, rho, n_samples=None if n_gl is None else win_hop * (n_gl - 1), N_out=win_hop * (T_s - 1))
        finally:
            gl_wav.free()   # (tts_free waits for the device: the resampling that reads it has run)
    return dict(wavs=finish(engine, wav, None if n_frames is None else win_hop * (np.asarray(n_frames, dtype=np.int32) - 1)))


@takes_settings()
def serve(sentence_generator, weights, dataset=None, device_id=0, pipelined=False, **settings):
    """Generator: for each batch of raw sentences yield the list of synthesized waveforms
    (reference tacotron/serve.py:89-126, with the SavedModel session replaced by the engine).

    Default: the reference's request/response order -- every batch is answered before the next one is pulled from
    ``sentence_generator`` (reference serve.py:108-124 blocks on a live generator, and a client may wait for its answer
    before it sends more).  ``pipelined=True`` keeps three batches in flight for OFFLINE streams whose batches are all
    available: batch k is then yielded only after batch k + 2 has been pulled from the generator (the last one when the
    generator ends), which on a request-driven generator would hold every answer back by two requests.
    ``settings``: the keywords of ``inference.SynthSettings`` -- with a loudness every answer of the stream
    comes at the same level, with a limiter under the same ceiling.  With ``check_alignment`` every answer is ``(waveforms, records, verdicts)`` -- the alignment
    records of the batch (``Engine.alignment_stats``) and ``attention_check.verdict`` of every utterance, in the same round trip
    as the waveforms: a bad utterance can be flagged before it is played.  With an ``output`` (``inference.SynthSettings``) every
    answer is in that sample format and at that rate -- 16-bit PCM, or G.711 at 8 kHz for telephony -- resampled and encoded on
    the device: pipelined, inside the call, so that only the codes cross the host boundary.  With ``marks`` ('word' or 'char')
    every answer gains, as its last element, the timing marks of every sentence (``tacotron.marks``; offsets into the raw
    sentence, samples of what is delivered): subtitles and barge-in positions in the same round trip as the waveforms."""
    # (a generator: a bad setting is refused at its first item, before a model is made)
    s = SynthSettings(model_params, **settings)
    dataset, model = open_model(weights, dataset, device_id)
    if not pipelined:   # the reference's loop as it stands: one batch at a time, spectrograms through host memory
        for k, sentences in enumerate(sentence_generator):
            ids = pre_process_sentences(sentences, dataset)
            texts = [(raw,) + marks_.token_spans(dataset, raw) for raw in sentences] if s.marks else None
            fetches = [model.output_linear_spec] + ([model.alignment_history] if s.check_alignment or s.marks else [])
            fetched = model.run(fetches, {model.inp_sentences: ids})
            wavs = post_process_spectrograms(fetched[0], model.engine, **s.keywords())
            held = [len(w) for w in wavs]   # (the samples every row holds at the model's rate)
            parts = dict(wavs=wavs if s.output is None else deliver(model.engine, wavs, s.output, seed=k))
            n_sent = model.engine.text_lengths(ids, pad_id()) if s.check_alignment or s.marks else None
            if s.check_alignment:   # (the same kernels as inside a pipelined call, on the alignments this loop fetched anyway)
                parts['records'] = model.engine.alignment_stats(fetched[1], n_sent=n_sent)
                parts['verdicts'] = attention_check.verdict(parts['records'])
            if s.marks:
                start, stats = model.engine.token_times(fetched[1], n_sent=n_sent, max_jump=s.marks_max_jump)
                parts['marks'] = marks_of_batch(model, s, ids, start, stats, held, parts['wavs'], texts)
            yield parts
        return
    # three batches in flight, nothing but ids and waveforms crosses the host boundary (inference.synthesize_stream)
    texts = []   # per batch pulled, what its marks take of the raw sentences

    def pulled():
        for sentences in sentence_generator:
            if s.marks:
                texts.append([(raw,) + marks_.token_spans(dataset, raw) for raw in sentences])
            yield pre_process_sentences(sentences, dataset)

    def pulled_texts():
        while True:
            yield texts.pop(0)

    for parts in synthesize_stream.parts(model, pulled(), peak_normalize=False, copy=True, mark_texts=pulled_texts(), **settings):
        parts['wavs'] = list(parts['wavs'])
        yield parts
