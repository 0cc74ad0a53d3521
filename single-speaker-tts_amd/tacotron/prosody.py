"""Prosody markup: per-word rate, volume, pitch and pauses inside a sentence (no reference counterpart).

A small subset of SSML -- ``<prosody rate=.. volume=..>``, ``<emphasis level=..>``, ``<break time=..|strength=../>`` under an
optional ``<speak>`` -- becomes the segment list of ``Engine.warp_magnitudes`` (tts_warp_magnitudes): ``parse_markup`` takes the
markup out of a sentence and keeps where it stood, ``token_attributes`` gives every token of the processed sentence its step and
gain, ``segments_of_row`` cuts an utterance's frames at the decoder steps ``Engine.token_times`` found for its tokens, and
``warp_position`` is the map from a source frame to its place in the warped utterance that the timing marks go through.
With ``pitch=True`` the parser also takes ``<prosody pitch=..>``: a token then carries the ratio 2 ** (-st / 12) of its span's
semitones beside a step that stretches it by that much more, ``pitch_segments_of_row`` turns the warp's segments into the sample
segments of ``Engine.resample_segments`` (tts_resample_segments), which takes Griffin-Lim's samples of the word back to the
duration it has without the pitch, and ``pitch_position`` is the map from a Griffin-Lim sample to its place in the retimed row.
With ``pitch_mode='envelope'`` the pitch is made ahead of Griffin-Lim on the frequency axis instead, where the formants stay put:
a token carries its semitones beside the step of the text without any pitch, and ``shift_segments_of_row`` turns the warp
segments' source ranges into the segments of ``Engine.shift_magnitudes`` (tts_shift_magnitudes); nothing is stretched or resampled.
Everything here is host arithmetic on a few integers.

What is NOT known: no trained checkpoint is at hand, so how any of this sounds on real speech has not been measured.  A border
between two rates is a decoder step -- r frames, 62.5 ms with r = 5 and 12.5 ms frames --, because that is the resolution of the
alignment; nothing is interpolated inside a step, and a gain changes at a border without a ramp.  Every preset below -- the
named rates, volumes and pitches, the emphasis levels, the pauses of the break strengths -- is UNTUNED: round figures, not
measured against recordings; so is the rounding of a pitch to a quarter of a semitone, which is there to keep the distinct
resampling ratios of a call few (each one below 1 has a table of its own on the device)."""
import math
import re
from xml.parsers import expat

import numpy as np

from . import marks as marks_
from .._hip import resample_segment_count, shift_step, warp_count

RATE_MIN, RATE_MAX = 0.25, 4.0          # the rates of tts_stretch_magnitudes and of a segment's step / 65536
GAIN_MAX = 16.0                         # the largest gain of a segment (+24.08 dB)
STEP_ONE = 65536
STEP_MIN, STEP_MAX = 16384, 262144      # the steps tts_warp_magnitudes takes
PITCH_MODES = ('resample', 'envelope')  # how a <prosody pitch=..> is made: behind Griffin-Lim on the samples, or ahead of it on the frequency axis

# UNTUNED presets (see the module's note)
RATES = {'x-slow': 0.5, 'slow': 0.75, 'medium': 1.0, 'fast': 1.25, 'x-fast': 1.5}
VOLUMES_DB = {'silent': -math.inf, 'x-soft': -12.0, 'soft': -6.0, 'medium': 0.0, 'loud': 6.0, 'x-loud': 12.0}
PITCHES_ST = {'x-low': -4.0, 'low': -2.0, 'medium': 0.0, 'high': 2.0, 'x-high': 4.0}
PITCH_MAX_ST = 12.0                     # the sum of the nested pitches, either way
PITCH_GRID_ST = 0.25                    # ... rounded to the nearest multiple of this
EMPHASIS = {'strong': (0.8, 3.0), 'moderate': (0.9, 1.5), 'reduced': (1.1, -3.0)}   # level -> (rate, volume in dB)
# a break's strength -> the kind of tacotron.inference.PAUSES_MS whose pause it takes (None: no pause)
BREAK_STRENGTHS = {'none': None, 'x-weak': None, 'weak': 'clause', 'medium': 'sentence', 'strong': 'sentence', 'x-strong': 'paragraph'}
BREAK_MAX_MS = 60000.0

_NUMBER = r'(?:\d+(?:\.\d*)?|\.\d+)'
_RATE_NUMBER = re.compile(r'^' + _NUMBER + r'$')
_RATE_PERCENT = re.compile(r'^(' + _NUMBER + r')%$')
_VOLUME_DB = re.compile(r'^([+-]' + _NUMBER + r')\s*dB$')
_PITCH_ST = re.compile(r'^([+-]' + _NUMBER + r')st$')
_PITCH_PERCENT = re.compile(r'^([+-]' + _NUMBER + r')%$')
_BREAK_TIME = re.compile(r'^(' + _NUMBER + r')(ms|s)$')


def _pauses_ms(pauses_ms):
    from .inference import PAUSES_MS   # (the table synthesize_text has; inference imports this module)
    table = dict(PAUSES_MS)
    table.update(pauses_ms or {})
    return table


def _rate(value, at):
    if value in RATES:
        return RATES[value]
    m = _RATE_PERCENT.match(value)
    rate = float(m.group(1)) / 100.0 if m else float(value) if _RATE_NUMBER.match(value) else None
    if rate is None or not rate > 0.0 or not math.isfinite(rate):
        raise ValueError('parse_markup: rate={!r} at offset {} is not a positive number, N% or one of {}'.format(value, at, ', '.join(RATES)))
    return rate


def _volume(value, at):
    if value in VOLUMES_DB:
        return VOLUMES_DB[value]
    m = _VOLUME_DB.match(value)
    if not m:
        raise ValueError('parse_markup: volume={!r} at offset {} is not +N dB, -N dB or one of {}'.format(value, at, ', '.join(VOLUMES_DB)))
    return float(m.group(1))


def _pitch(value, at):
    """a pitch= value in semitones: +Nst / -Nst, +N% / -N% (12 log2(1 + N / 100)) or a preset"""
    if value in PITCHES_ST:
        return PITCHES_ST[value]
    m = _PITCH_ST.match(value)
    if m:
        return float(m.group(1))
    m = _PITCH_PERCENT.match(value)
    factor = 1.0 + float(m.group(1)) / 100.0 if m else None
    if factor is None or not factor > 0.0:
        raise ValueError('parse_markup: pitch={!r} at offset {} is not +Nst, -Nst, +N%, -N% (above -100%) or one of {}{}'.format(
            value, at, ', '.join(PITCHES_ST), ' (a pitch in Hz is not supported: the voice\'s own pitch is not known)' if value.endswith('Hz') else ''))
    return 12.0 * math.log2(factor)


def round_semitones(st):
    """a sum of pitches on the quarter-semitone grid: the nearest multiple of PITCH_GRID_ST, a tie away from zero"""
    q = math.floor(abs(float(st)) / PITCH_GRID_ST + 0.5) * PITCH_GRID_ST
    return math.copysign(q, st) if q else 0.0


def pitch_ratio(semitones):
    """the resampling ratio of a segment ``semitones`` up: 2 ** (-st / 12) output samples per input sample"""
    return 2.0 ** (-float(semitones) / 12.0)


def parse_markup(text, pauses_ms=None, pitch=False):
    """``(plain, spans, breaks)`` of a marked sentence.  ``plain``: the text with the markup removed.  ``spans``: one ``(start, end,
    rate, volume_db)`` per ``<prosody>`` or ``<emphasis>`` element, in document order (an outer element in front of those inside
    it), offsets into ``plain``, ``rate`` the product of the element's rate with those around it and ``volume_db`` the sum of the
    volumes in dB (-inf: silent).  ``breaks``: ``(offset, ms)`` per ``<break/>``, the pause in front of ``plain[offset]``.

    Accepted, nested freely, under an optional ``<speak>`` root: ``<prosody rate=.. volume=..>`` -- rate a number, ``N%`` or x-slow,
    slow, medium, fast, x-fast; volume ``+N dB`` / ``-N dB`` or silent, x-soft, soft, medium, loud, x-loud --, ``<emphasis
    level="strong|moderate|reduced">`` (no level: moderate) and ``<break time="Nms|Ns"/>`` or ``<break strength="none|x-weak|weak|
    medium|strong|x-strong"/>`` (neither: medium), a strength taking the pause of ``pauses_ms`` over tacotron.inference.PAUSES_MS:
    weak the clause's, medium and strong the sentence's, x-strong the paragraph's.  ``&lt;``, ``&gt;``, ``&amp;``, ``&quot;`` and
    ``&apos;`` stand for their characters.  Anything else -- an unknown element or attribute, a value that cannot be read, tags
    that do not balance -- is a ValueError that names the thing and its offset in ``text``.

    ``pitch``: ``<prosody pitch=..>`` is accepted too -- ``+Nst`` / ``-Nst`` semitones, ``+N%`` / ``-N%`` (12 log2(1 + N / 100)
    semitones) or x-low, low, medium, high, x-high (-4, -2, 0, +2, +4 semitones) -- and a span is ``(start, end, rate, volume_db,
    semitones)``: the sum of the element's pitch with those around it, rounded to the nearest quarter of a semitone, which must
    lie in [-12, 12]; ``<emphasis>`` keeps its meaning and the pitch around it.  A value in ``Hz`` is refused with its offset.
    Without ``pitch`` the attribute is unknown, as before."""
    if not isinstance(text, str):
        raise ValueError('parse_markup: a string is needed, got {!r}'.format(type(text).__name__))
    pauses = None
    head = '<markup>'
    data = (head + text + '</markup>').encode('utf-8')
    parser = expat.ParserCreate('utf-8')
    plain, spans, breaks = [], [], []
    stack = []          # per open element: (name, rate, volume_db, index into spans or None, semitones before rounding)
    state = dict(n=0, speak=0)      # speak: <speak> roots seen
    rooted = re.match(r'\s*<speak[\s>/]', text) is not None

    def offset():
        return max(0, len(data[:parser.CurrentByteIndex].decode('utf-8', errors='ignore')) - len(head))

    def start(name, attrs):
        nonlocal pauses
        at = offset()
        if name == 'markup' and not stack:
            stack.append((name, 1.0, 0.0, None, 0.0))
            return
        if stack and stack[-1][0] == 'break':
            raise ValueError('parse_markup: <break> at offset {} must be empty, it holds <{}>'.format(at, name))
        _n, rate, volume, _i, semis = stack[-1]
        known = {'speak': (), 'prosody': ('rate', 'volume', 'pitch') if pitch else ('rate', 'volume'), 'emphasis': ('level',), 'break': ('time', 'strength')}
        if name not in known:
            raise ValueError('parse_markup: unknown element <{}> at offset {}'.format(name, at))
        for key in attrs:
            if key not in known[name]:
                raise ValueError('parse_markup: unknown attribute {}= of <{}> at offset {}'.format(key, name, at))
        if name == 'speak':
            if len(stack) != 1 or state['speak'] or not rooted:
                raise ValueError('parse_markup: <speak> at offset {} is not the root'.format(at))
            state['speak'] = 1
            stack.append((name, rate, volume, None, semis))
            return
        if rooted and len(stack) == 1:
            raise ValueError('parse_markup: <{}> at offset {} stands outside <speak>'.format(name, at))
        if name == 'break':
            if 'time' in attrs and 'strength' in attrs:
                raise ValueError('parse_markup: <break> at offset {} has both time= and strength='.format(at))
            if 'time' in attrs:
                m = _BREAK_TIME.match(attrs['time'])
                ms = float(m.group(1)) * (1000.0 if m.group(2) == 's' else 1.0) if m else None
                if ms is None or not ms <= BREAK_MAX_MS:
                    raise ValueError('parse_markup: time={!r} at offset {} is not Nms or Ns of at most {:g} s'.format(attrs['time'], at, BREAK_MAX_MS / 1000.0))
            else:
                strength = attrs.get('strength', 'medium')
                if strength not in BREAK_STRENGTHS:
                    raise ValueError('parse_markup: strength={!r} at offset {} is not one of {}'.format(strength, at, ', '.join(BREAK_STRENGTHS)))
                pauses = _pauses_ms(pauses_ms) if pauses is None else pauses
                kind = BREAK_STRENGTHS[strength]
                ms = 0.0 if kind is None else float(pauses[kind])
            breaks.append((state['n'], ms))
            stack.append((name, rate, volume, None, semis))
            return
        if name == 'prosody':
            if 'rate' in attrs:
                rate = rate * _rate(attrs['rate'], at)
            if 'volume' in attrs:
                volume = volume + _volume(attrs['volume'], at)
            if 'pitch' in attrs:
                semis = semis + _pitch(attrs['pitch'], at)
                if not abs(round_semitones(semis)) <= PITCH_MAX_ST:
                    raise ValueError('parse_markup: pitch={!r} at offset {} brings the pitch to {:+g} semitones, which is not in [-12, 12]'.format(
                        attrs['pitch'], at, round_semitones(semis)))
        else:
            level = attrs.get('level', 'moderate')
            if level not in EMPHASIS:
                raise ValueError('parse_markup: level={!r} at offset {} is not one of {}'.format(level, at, ', '.join(EMPHASIS)))
            rate, volume = rate * EMPHASIS[level][0], volume + EMPHASIS[level][1]
        spans.append([state['n'], None, rate, volume] + ([round_semitones(semis)] if pitch else []))
        stack.append((name, rate, volume, len(spans) - 1, semis))

    def end(name):
        _n, _r, _v, i, _s = stack.pop()
        if i is not None:
            spans[i][1] = state['n']

    def chars(s):
        at = offset()
        if stack[-1][0] == 'break':
            raise ValueError('parse_markup: <break> at offset {} must be empty'.format(at))
        if rooted and len(stack) == 1:      # (around the <speak> root: blanks alone)
            if s.strip():
                raise ValueError('parse_markup: text at offset {} stands outside <speak>'.format(at))
            return
        plain.append(s)
        state['n'] += len(s)

    parser.StartElementHandler, parser.EndElementHandler, parser.CharacterDataHandler = start, end, chars
    try:
        parser.Parse(data, True)
    except expat.ExpatError as e:
        at = max(0, len(data[:parser.ErrorByteIndex].decode('utf-8', errors='ignore')) - len(head))
        raise ValueError('parse_markup: malformed markup at offset {}: {}'.format(min(at, len(text)), expat.ErrorString(e.code)))
    return ''.join(plain), [tuple(s) for s in spans], breaks


def volume_gain(volume_db):
    """a volume in dB as the float32 gain of a segment: 10 ** (dB / 20), 0 for -inf"""
    return np.float32(0.0) if volume_db == -math.inf else np.float32(10.0 ** (float(volume_db) / 20.0))


def break_frames(ms, hop, sampling_rate):
    """a pause of ``ms`` milliseconds in frames of ``hop`` samples: rounded to the nearest, at least one where ms > 0"""
    if not ms > 0.0:
        return 0
    return max(1, int(math.floor(float(ms) * float(sampling_rate) / (1000.0 * float(hop)) + 0.5)))


def token_attributes(dataset, plain, spans, breaks, base_rate=1.0, hop=275, sampling_rate=22050, pitch=False, pitch_mode='resample'):
    """``(attrs, token_breaks)`` of a parsed sentence.  ``attrs``: one ``(step, gain)`` per token of the processed sentence --
    ``marks.token_spans``: lower case, abbreviations expanded -- and a last one for the end token, which carries the base
    attributes: ``step = round(65536 * base_rate * rate)`` and ``gain`` the float32 of 10 ** (volume_db / 20).  A token takes
    the innermost span that holds ALL of the raw characters it came from, so the expansion of an abbreviation belongs to the span
    that holds the abbreviation, and a span that ends inside one does not reach it.  ``token_breaks``: ``(token, frames)`` per
    break of at least one frame (``break_frames``), the pause in front of that token -- the first one that starts at or behind
    the break's offset, the end token where there is none --, breaks in front of one token added up.  ValueError, naming the
    span, for a product of rates outside [0.25, 4] or a gain above 16.

    ``pitch``: the spans are ``parse_markup(.., pitch=True)``'s, with their semitones ``st``, and an attribute is ``(step, gain,
    ratio)``: ``step = round(65536 * base_rate * rate * 2 ** (-st / 12))`` -- the warp stretches the token's frames by a further
    2 ** (-st / 12) -- and ``ratio = 2.0 ** (-st / 12.0)``, at which ``Engine.resample_segments`` takes the token's samples back
    to the duration they have without the pitch (1.0 where there is none).  ValueError, naming the span, for a step outside
    [16384, 262144].

    ``pitch_mode`` 'envelope' (with ``pitch``): the pitch is made on the frequency axis (``Engine.shift_magnitudes``), so nothing is
    stretched and an attribute is ``(step, gain, st)``: the step of the call without any pitch, ``round(65536 * base_rate * rate)``,
    and the span's semitones (0.0 where there is none).  'resample' (the default): as above."""
    if pitch_mode not in PITCH_MODES:
        raise ValueError('token_attributes: pitch_mode must be one of {}, got {!r}'.format(PITCH_MODES, pitch_mode))
    envelope = bool(pitch) and pitch_mode == 'envelope'
    base = float(base_rate)
    if not RATE_MIN <= base <= RATE_MAX:
        raise ValueError('token_attributes: the base rate must lie in [0.25, 4], got {!r}'.format(base_rate))
    processed, tok = marks_.token_spans(dataset, plain)
    one = (int(math.floor(STEP_ONE * base + 0.5)), np.float32(1.0)) + (((0.0,) if envelope else (1.0,)) if pitch else ())
    attrs = [one] * (len(processed) + 1)
    for k, span in enumerate(spans):
        a, b, rate, volume_db = span[:4]
        what = 'span {} ({!r}, characters {} .. {})'.format(k, plain[a:b], a, b)
        product = base * float(rate)
        if not RATE_MIN <= product <= RATE_MAX:
            raise ValueError('token_attributes: {} has rate {:g} x {:g} = {:g}, which is not in [0.25, 4]'.format(what, base, float(rate), product))
        gain = volume_gain(volume_db)
        if not gain <= GAIN_MAX:
            raise ValueError('token_attributes: {} has volume {:+g} dB, a gain above 16'.format(what, volume_db))
        value = (int(math.floor(STEP_ONE * product + 0.5)), gain)
        if envelope:
            value = value + (float(span[4]),)
        elif pitch:
            ratio = pitch_ratio(span[4])
            step = int(math.floor(STEP_ONE * product * ratio + 0.5))
            if not STEP_MIN <= step <= STEP_MAX:
                raise ValueError('token_attributes: {} has rate {:g} at {:+g} semitones: the step {} is not in {} .. {}'.format(
                    what, product, span[4], step, STEP_MIN, STEP_MAX))
            value = (step, gain, ratio)
        for j, (s, e) in enumerate(tok):
            if a <= s and e <= b:
                attrs[j] = value
    pauses = {}
    for at, ms in breaks:
        frames = break_frames(ms, hop, sampling_rate)
        if frames:
            j = next((j for j, (s, _e) in enumerate(tok) if s >= at), len(processed))
            pauses[j] = pauses.get(j, 0) + frames
    return attrs, sorted(pauses.items())


def segments_of_row(start, n_sent, r, n_frames, attrs, breaks, min_frames=1, row=0):
    """The segments of one utterance, rows ``(row, first, frames, pause, step, gain)`` of ``Engine.warp_magnitudes``, and its
    ``n_out``.  ``start``: the row of tts_token_times -- token j of the ``n_sent`` tokens (the end token is the last) owns the
    source frames [r * start[j], r * start[j + 1]), clipped to the ``n_frames`` the utterance holds (the end-of-speech cut); a
    token without a step contributes nothing; neighbouring tokens of equal ``(step, gain)`` (``attrs``, one per token) merge into
    one segment; a break ``(token, frames)`` becomes a pause in front of its token (a break behind the cut: at the end), pauses
    that meet become one; and a trailing pause pads a row whose ``n_out`` would fall below ``min_frames`` (Griffin-Lim's least,
    speech_min_frames).

    Attributes ``(step, gain, ratio)`` (``token_attributes(.., pitch=True)``): neighbouring tokens merge only where their ratios
    are equal too, and a third element is returned, the ratio of every segment (1.0 for a pause)."""
    n_sent, r, n_frames = int(n_sent), int(r), int(n_frames)
    if len(start) < n_sent + 1 or len(attrs) != n_sent:
        raise ValueError('segments_of_row: {} tokens need {} start steps and {} attributes, got {} and {}'.format(
            n_sent, n_sent + 1, n_sent, len(start), len(attrs)))
    if n_frames < 1 or r < 1:
        raise ValueError('segments_of_row: need n_frames, r >= 1, got {}, {}'.format(n_frames, r))
    pause_at = {}
    for j, frames in breaks:
        if not 0 <= j < n_sent or frames < 1:
            raise ValueError('segments_of_row: a break ({}, {}) of {} tokens'.format(j, frames, n_sent))
        pause_at[int(j)] = pause_at.get(int(j), 0) + int(frames)
    seg, ratios = [], []
    pitched = len(attrs) > 0 and len(attrs[0]) == 3

    def pause(frames):
        if seg and seg[-1][2] == 0:
            seg[-1][3] += frames
        else:
            seg.append([row, 0, 0, frames, 0, np.float32(0.0)])
            ratios.append(1.0)

    for j in range(n_sent):
        if j in pause_at:
            pause(pause_at[j])
        a, b = min(r * int(start[j]), n_frames), min(r * int(start[j + 1]), n_frames)
        if b <= a:
            continue
        step, gain = int(attrs[j][0]), np.float32(attrs[j][1])
        ratio = float(attrs[j][2]) if pitched else 1.0
        if seg and seg[-1][2] > 0 and seg[-1][1] + seg[-1][2] == a and seg[-1][4] == step and seg[-1][5] == gain and ratios[-1] == ratio:
            seg[-1][2] += b - a
        else:
            seg.append([row, a, b - a, 0, step, gain])
            ratios.append(ratio)
    n_out = sum(q[3] if q[2] == 0 else warp_count(q[2], q[4]) for q in seg)
    if n_out < min_frames:
        pause(int(min_frames) - n_out)
        n_out = int(min_frames)
    rows = [(q[0], q[1], q[2], q[3], q[4], float(q[5])) for q in seg]
    return (rows, n_out, ratios) if pitched else (rows, n_out)


def warp_position(segments, frame, side='right'):
    """Where source frame ``frame`` (a float) of an utterance lies in its warped output, in output frames (float64): the
    piecewise-linear map that takes the source range of every speech segment of ``segments`` -- one row's, in source order, as
    ``segments_of_row`` makes them -- onto the output frames the segment fills, ``o + count * (frame - first) / frames``.  It is
    monotone, continuous from one speech segment into the next and jumps across a pause: at such a border ``side`` 'right'
    (where something starts) gives the position behind the pause, 'left' (where something ends) the one in front of it.  A frame
    at or behind the last speech segment's end: ``n_out`` ('right'), the end of that segment ('left')."""
    if side not in ('right', 'left'):
        raise ValueError("warp_position: side must be 'right' or 'left', got {!r}".format(side))
    x = float(frame)
    o, before = 0, 0.0          # output frames so far; ... up to the end of the last speech segment
    for _row, first, frames, pause, step, _gain in segments:
        if frames == 0:
            o += int(pause)
            continue
        count = warp_count(frames, step)
        if side == 'left' and x <= first:
            return before
        if x < first:
            return float(o)
        if x < first + frames or (side == 'left' and x == first + frames):
            return float(o) + (float(count) * (x - float(first))) / float(frames)
        o += count
        before = float(o)
    return float(o) if side == 'right' else before


def pitch_segments_of_row(warp_segments, ratios, hop, n_out, row=0):
    """The segments of one utterance for ``Engine.resample_segments``, rows ``(row, first, samples, ratio)``, and the samples the
    retimed row holds.  ``warp_segments`` / ``ratios``: ``segments_of_row``'s -- segment s owns the output frames [o, o + count) of
    the warp, which Griffin-Lim turns into the samples [hop * o, hop * (o + count)), clipped to the hop * (n_out - 1) the row
    holds, and they are resampled at ``ratios[s]`` (a pause: 1.0, a copy); a segment the clip leaves nothing of is dropped, and
    neighbours of equal ratio merge -- a row without a pitch is one copy of itself."""
    if len(ratios) != len(warp_segments):
        raise ValueError('pitch_segments_of_row: {} segments need {} ratios, got {}'.format(len(warp_segments), len(warp_segments), len(ratios)))
    hop, held = int(hop), int(hop) * (int(n_out) - 1)
    if held < 1:
        raise ValueError('pitch_segments_of_row: a row of {} frames holds no sample'.format(n_out))
    seg, o = [], 0
    for (_row, _first, frames, pause, step, _gain), ratio in zip(warp_segments, ratios):
        count = int(pause) if frames == 0 else warp_count(frames, step)
        a, b = min(hop * o, held), min(hop * (o + count), held)
        o += count
        if b <= a:
            continue
        ratio = 1.0 if frames == 0 else float(ratio)
        if seg and seg[-1][3] == ratio:
            seg[-1][2] += b - a
        else:
            seg.append([row, a, b - a, ratio])
    if o != int(n_out):
        raise ValueError('pitch_segments_of_row: the segments make {} frames, the row has {}'.format(o, n_out))
    return [tuple(q) for q in seg], sum(resample_segment_count(q[2], q[3]) for q in seg)


def shift_segments_of_row(warp_segments, semitones, timbre_st=0.0, row=0):
    """The segments of one utterance for ``Engine.shift_magnitudes``, rows ``(row, first, frames, pitch_step, formant_step)``.
    ``warp_segments`` / ``semitones``: ``segments_of_row``'s under ``token_attributes(.., pitch_mode='envelope')`` -- the SOURCE
    frames [first, first + frames) of every speech segment (already clipped at the end-of-speech cut) get ``shift_step(st)`` for
    the fine structure and ``shift_step(timbre_st)`` for the envelope, ``timbre_st`` the same for every frame; a pause has no
    source frames and is skipped, and neighbours that touch and have equal steps merge.  The shift runs ahead of the warp, on the
    frames the network made.  ValueError for semitones outside -12 .. 12."""
    if len(semitones) != len(warp_segments):
        raise ValueError('shift_segments_of_row: {} segments need {} pitches, got {}'.format(len(warp_segments), len(warp_segments), len(semitones)))
    formant = shift_step(timbre_st)
    seg = []
    for (_row, first, frames, _pause, _step, _gain), st in zip(warp_segments, semitones):
        if frames == 0:
            continue
        step = shift_step(st)
        if seg and seg[-1][1] + seg[-1][2] == first and seg[-1][3] == step:
            seg[-1][2] += frames
        else:
            seg.append([row, int(first), int(frames), step, formant])
    return [tuple(q) for q in seg]


def pitch_position(segments, sample, side='right'):
    """Where Griffin-Lim's sample ``sample`` (a float) of an utterance lies in its retimed row, in samples (float64): the
    piecewise-linear map that takes the source range of every segment of ``segments`` -- one row's, as ``pitch_segments_of_row``
    makes them: in source order, each starting where the last one ended -- onto the samples the segment fills, ``o + count *
    (sample - first) / samples``.  ``warp_position``'s counterpart with the same ``side`` rule; the segments leave no gap, so the
    map is monotone and continuous and both sides agree.  A sample at or behind the last segment's end: the row's length."""
    if side not in ('right', 'left'):
        raise ValueError("pitch_position: side must be 'right' or 'left', got {!r}".format(side))
    x = float(sample)
    o, before = 0, 0.0
    for _row, first, samples, ratio in segments:
        count = resample_segment_count(samples, ratio)
        if side == 'left' and x <= first:
            return before
        if x < first:
            return float(o)
        if x < first + samples or (side == 'left' and x == first + samples):
            return float(o) + (float(count) * (x - float(first))) / float(samples)
        o += count
        before = float(o)
    return float(o) if side == 'right' else before
