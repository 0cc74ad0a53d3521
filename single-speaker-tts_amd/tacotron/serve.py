"""Mirror of the reference's serving helpers (tacotron/serve.py:22-126) on the MI355X path.

``pre_process_sentences`` (:22-36) and ``post_process_spectrograms`` (:39-86) keep their names;
``serve`` (:89-126) is the same loop -- sentences from a generator, one batch per iteration --
driving the HIP library instead of a TensorFlow SavedModel session.  Unlike the reference's
``post_process_spectrograms`` (which squeezes a trailing axis and therefore only works for a batch
of one, serve.py:58), a whole batch is supported.
"""
import numpy as np

from .._hip import limiter_lookahead, synth_frame_counts, synth_lengths
from ..audio.conversion import ms_to_samples
from . import attention_check, marks as marks_
from .inference import SILENCE_KEEP_MS, SynthSettings, cut_waveforms, deliver, marks_of_batch, pad_id, pad_sentence, synthesize_stream
from .model import Mode, Tacotron
from .params import dataset_params, model_params


def pre_process_sentences(_sentences, dataset):
    """raw strings -> padded int32 id batch (reference tacotron/serve.py:22-36)."""
    id_sequences, sequence_lengths = dataset.process_sentences(_sentences)
    sentences = [np.frombuffer(s, dtype=np.int32) for s in id_sequences]
    max_length = max(sequence_lengths)
    return np.array([pad_sentence(s, max_length) for s in sentences], dtype=np.int32)


def post_process_spectrograms(_spectrograms, engine, init_phase=None, seed=0, momentum=0.0, stop_at_silence_db=None,
                              silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0, phase_init='random',
                              loudness=None, limiter=None):
    """normalised linear spectrograms (B, T, 1025) -> list of waveforms: de-normalise with the mel dB
    constants, ``** magnitude_power``, Griffin-Lim (reference tacotron/serve.py:39-86).  The settings from ``momentum`` on mean
    what ``inference.SynthSettings`` says, composed here from the engine's stages: with ``stop_at_silence_db``
    ``Engine.speech_frames`` on the normalised spectrograms, then one ragged Griffin-Lim call, every utterance returned at its own
    length; with a ``speaking_rate`` or a ``pitch`` ``Engine.stretch_magnitudes`` by rate * 2 ** -pitch ahead of Griffin-Lim
    (``init_phase`` has that many frames; lengths min(T', max(min_frames, ceil(n / rate)))) and ``Engine.resample`` by 2 ** -pitch
    behind it; with a ``loudness`` ``Engine.loudness_normalize``, every waveform measured over its own samples; with a ``limiter`` ``Engine.limit``
    last, over the same samples."""
    s = SynthSettings(model_params, momentum, stop_at_silence_db, silence_keep_ms, speaking_rate, pitch, phase_init, loudness, limiter=limiter)
    stop, rate, octaves, loud = s.stop, s.rate, s.octaves, s.loud
    lookahead = None if s.limiter is None else limiter_lookahead('post_process_spectrograms', s.limiter[1], model_params.sampling_rate)
    rho = float(np.exp2(-np.float64(octaves)))
    loader = dataset_params.dataset_loader
    win_len = ms_to_samples(model_params.win_len, model_params.sampling_rate)
    win_hop = ms_to_samples(model_params.win_hop, model_params.sampling_rate)
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
        thr = engine.speech_threshold(stop[0], loader.mel_mag_ref_db, loader.mel_mag_max_db)
        n_frames = engine.speech_frames(spec, thr, keep_frames=stop[1], min_frames=min_frames)[0].to_host()
    mag = engine.denorm_power(spec, loader.mel_mag_ref_db, loader.mel_mag_max_db, model_params.magnitude_power)
    n_gl = n_frames   # the frames Griffin-Lim runs on
    if rate != 1.0 or octaves != 0.0:
        mag = engine.stretch_magnitudes(mag, rate * rho, n_frames=n_frames, T_out=T_g)
        if n_frames is not None:
            n_frames, n_gl = synth_lengths(n_frames, T, rate, octaves, min_frames)
    wav, _ = engine.griffin_lim(mag, model_params.reconstruction_iterations, win_len, win_hop, model_params.n_fft,
                                init_phase=init_phase, seed=seed, want_mse=False, momentum=momentum, n_frames=n_gl,
                                phase_init=phase_init)
    if octaves != 0.0:
        gl_wav = wav
        try:
            wav = engine.resample(gl_wav, rho, n_samples=None if n_gl is None else win_hop * (n_gl - 1), N_out=win_hop * (T_s - 1))
        finally:
            gl_wav.free()   # (tts_free waits for the device: the resampling that reads it has run)
    held = None if n_frames is None else win_hop * (np.asarray(n_frames, dtype=np.int32) - 1)
    if loud is not None:
        engine.loudness_normalize(wav, model_params.sampling_rate, loud[0], loud[1], n_samples=held)
    if s.limiter is not None:
        engine.limit(wav, s.limiter[0], lookahead, s.limiter[2], n_samples=held)
    wav = wav.to_host()
    if n_frames is not None:
        return cut_waveforms(wav, n_frames, win_hop)
    return [wav[b] for b in range(wav.shape[0])]


def serve(sentence_generator, weights, dataset=None, device_id=0, pipelined=False, momentum=0.0, stop_at_silence_db=None,
          silence_keep_ms=SILENCE_KEEP_MS, speaking_rate=1.0, pitch=0.0, phase_init='random', loudness=None,
          check_alignment=False, limiter=None, output=None, marks=None, marks_max_jump=4):
    """Generator: for each batch of raw sentences yield the list of synthesized waveforms
    (reference tacotron/serve.py:89-126, with the SavedModel session replaced by the engine).

    Default: the reference's request/response order -- every batch is answered before the next one is pulled from
    ``sentence_generator`` (reference serve.py:108-124 blocks on a live generator, and a client may wait for its answer
    before it sends more).  ``pipelined=True`` keeps three batches in flight for OFFLINE streams whose batches are all
    available: batch k is then yielded only after batch k + 2 has been pulled from the generator (the last one when the
    generator ends), which on a request-driven generator would hold every answer back by two requests.
    The settings from ``momentum`` on: as ``inference.SynthSettings`` has them -- with a loudness every answer of the stream
    comes at the same level, with a limiter under the same ceiling.  With ``check_alignment`` every answer is ``(waveforms, records, verdicts)`` -- the alignment
    records of the batch (``Engine.alignment_stats``) and ``attention_check.verdict`` of every utterance, in the same round trip
    as the waveforms: a bad utterance can be flagged before it is played.  With an ``output`` (``inference.SynthSettings``) every
    answer is in that sample format and at that rate -- 16-bit PCM, or G.711 at 8 kHz for telephony -- resampled and encoded on
    the device: pipelined, inside the call, so that only the codes cross the host boundary.  With ``marks`` ('word' or 'char')
    every answer gains, as its last element, the timing marks of every sentence (``tacotron.marks``; offsets into the raw
    sentence, samples of what is delivered): subtitles and barge-in positions in the same round trip as the waveforms."""
    # (a generator: a bad setting is refused at its first item, before a model is made)
    s = SynthSettings(model_params, momentum, stop_at_silence_db, silence_keep_ms, speaking_rate, pitch, phase_init, loudness, check_alignment,
                      limiter=limiter, output=output, marks=marks, marks_max_jump=marks_max_jump)
    from ..datasets.lj_speech import LJSpeechDatasetHelper
    dataset = dataset or LJSpeechDatasetHelper(dataset_folder=dataset_params.dataset_folder,
                                                char_dict=dataset_params.vocabulary_dict, fill_dict=False)
    model = Tacotron(inputs=Tacotron.model_placeholders(), mode=Mode.PREDICT, weights=weights, device_id=device_id)
    if not pipelined:   # the reference's loop as it stands: one batch at a time, spectrograms through host memory
        for k, sentences in enumerate(sentence_generator):
            ids = pre_process_sentences(sentences, dataset)
            texts = [(raw,) + marks_.token_spans(dataset, raw) for raw in sentences] if s.marks else None
            fetches = [model.output_linear_spec] + ([model.alignment_history] if check_alignment or s.marks else [])
            fetched = model.run(fetches, {model.inp_sentences: ids})
            wavs = post_process_spectrograms(fetched[0], model.engine, **s.keywords())
            held = [len(w) for w in wavs]   # (the samples every row holds at the model's rate)
            if s.output is not None:
                wavs = deliver(model.engine, wavs, s.output, seed=k)
            answer = (wavs,)
            n_sent = model.engine.text_lengths(ids, pad_id()) if check_alignment or s.marks else None
            if check_alignment:   # (the same kernels as inside a pipelined call, on the alignments this loop fetched anyway)
                records = model.engine.alignment_stats(fetched[1], n_sent=n_sent)
                answer += (records, attention_check.verdict(records))
            if s.marks:
                start, stats = model.engine.token_times(fetched[1], n_sent=n_sent, max_jump=s.marks_max_jump)
                answer += (marks_of_batch(model, s, ids, start, stats, held, wavs, texts),)
            yield answer if len(answer) > 1 else wavs
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

    for item in synthesize_stream(model, pulled(), peak_normalize=False, copy=True, check_alignment=check_alignment, output=output,
                                  marks=marks, marks_max_jump=marks_max_jump, mark_texts=pulled_texts(), **s.keywords()):
        wavs = item[0] if check_alignment or s.marks else item
        listed = [wavs[b] for b in range(len(wavs))]
        yield ((listed,) + tuple(item[1:])) if check_alignment or s.marks else listed
