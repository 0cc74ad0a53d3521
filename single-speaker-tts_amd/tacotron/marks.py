"""Timing marks: when every word of a synthesized text is spoken (no reference counterpart).

``Engine.token_times`` (tts_token_times) turns a call's alignments into ``start``: token j of an utterance is spoken during the
decoder steps ``start[j] .. start[j + 1]``.  Everything here is host arithmetic in float64 on those few integers: which tokens
make a word and where they came from in the raw text (``token_spans``), where a step border lies in the samples the caller
receives (``step_sample`` -- through the reduction factor, the hop, the speaking rate and the end-of-speech cut -- then
``marks_of_text`` through the lead trim, the pauses and cross-fades of the join and the parts of a text that span calls, then the
output rate), and the marks as JSON lines (``write_marks``).

What is NOT known: no trained checkpoint is at hand, so how well the marks sit on real speech has not been measured.  A border
is a decoder step, r * hop samples (62.5 ms with r = 5 and 12.5 ms frames): nothing is interpolated inside a step.  ``max_jump``
(four tokens a step) and ``reliable`` (the path agrees with the plain argmax at half of the steps) are untuned heuristics."""
import json

import numpy as np

KINDS = ('word', 'char')
RELIABLE_AGREE = 0.5   # untuned: the share of the steps at which the path stands on the row's argmax


def marks_kind(marks):
    """``marks`` of the helpers of ``tacotron.inference`` -- None, 'word' or 'char' -- checked; ValueError for anything else"""
    if marks is not None and marks not in KINDS:
        raise ValueError("marks must be None, 'word' or 'char', got {!r}".format(marks))
    return marks


def reliable(stats):
    """True where the monotone path of an utterance stands on the argmax of its row at half of its steps or more
    (``agree / n_steps >= 0.5``): an UNTUNED heuristic.  A flat or wandering attention -- the reference's own dumped alignment --
    gives a path, because the search always gives one, and fails this."""
    return bool(float(stats['agree']) / float(stats['n_steps']) >= RELIABLE_AGREE)


def token_spans(dataset, sentence):
    """``(processed, spans)``: ``processed`` is the string ``dataset.process_sentences`` encodes -- lower case, abbreviations
    replaced in the dict's order --, and ``spans[i]`` the ``(start, end)`` in the RAW ``sentence`` that processed character i came
    from; every character of an expansion maps to its abbreviation's span.  ValueError where no map can be built (a character
    whose lower case is not one character) or the string is not the front end's."""
    lowered = sentence.lower()
    if len(lowered) != len(sentence):
        raise ValueError('token_spans: lower case changes the length of {!r}: no map to the raw text'.format(sentence))
    chars = list(lowered)
    spans = [(i, i + 1) for i in range(len(chars))]
    for abbreviation, expansion in getattr(dataset, '_abbreviations', {}).items():
        if not abbreviation:
            raise ValueError('token_spans: an empty abbreviation has no span')
        text, n = ''.join(chars), len(abbreviation)
        new_chars, new_spans, at = [], [], 0
        while True:                                  # (str.replace: left to right, no overlaps)
            hit = text.find(abbreviation, at)
            if hit < 0:
                break
            new_chars += chars[at:hit]
            new_spans += spans[at:hit]
            span = (min(s for s, _e in spans[hit:hit + n]), max(e for _s, e in spans[hit:hit + n]))
            new_chars += list(expansion)
            new_spans += [span] * len(expansion)
            at = hit + n
        chars, spans = new_chars + chars[at:], new_spans + spans[at:]
    processed = ''.join(chars)
    if processed != dataset.replace_abbreviations(lowered):
        raise ValueError('token_spans: {!r} is not what the front end makes of {!r}'.format(processed, sentence))
    return processed, spans


def ids_text(ids, n_sent, vocabulary):
    """``(processed, spans)`` of a row of ids for callers that never saw the text: the characters of its first ``n_sent - 1``
    ids by ``vocabulary`` (character -> id; the row's last token is the end token), an id without a one-character name as '?',
    and ``spans[i] = (i, i + 1)``: offsets into that string, not into a raw text"""
    names = {int(i): c for c, i in vocabulary.items()}
    chars = [names.get(int(i), '?') for i in list(ids)[:max(int(n_sent) - 1, 0)]]
    processed = ''.join(c if len(c) == 1 else '?' for c in chars)
    return processed, [(i, i + 1) for i in range(len(processed))]


def piece_spans(dataset, text, start, end):
    """``(processed, spans)`` of the piece ``text[start:end]`` of a text (``datasets.text_split.split_text_spans``: the piece is
    that slice with its whitespace runs collapsed) with the spans in ``text`` itself: ``token_spans`` of the collapsed piece,
    taken back through the collapse -- a blank of the piece is the whole whitespace run it came from"""
    back, i = [], start
    while i < end:
        j = i + 1
        if text[i].isspace():
            while j < end and text[j].isspace():
                j += 1
        back.append((i, j))
        i = j
    processed, spans = token_spans(dataset, ' '.join(text[start:end].split()))
    return processed, [(back[a][0], back[b - 1][1]) for a, b in spans]


def step_sample(k, r, hop, rate, n_held):
    """Where step border k lies in a row of the call, in samples (float64): at network frame r * k, at stretched frame r * k /
    rate, at sample hop * r * k / rate -- and not behind the ``n_held = hop * (n_frames[b] - 1)`` samples the row holds.  The pitch
    moves nothing (the resampler takes its samples back), nor do the loudness gain and the limiter."""
    return min(float(hop) * float(r) * float(k) / float(rate), float(n_held))


def out_sample(x, rate_in, rate_out, n_out):
    """a position in samples at ``rate_in`` as a sample at ``rate_out``: floor(x * rate_out / rate_in + 0.5), within 0 .. n_out"""
    return int(min(max(np.floor(float(x) * float(rate_out) / float(rate_in) + 0.5), 0.0), float(n_out)))


def words_of(processed):
    """the maximal runs of non-blank characters of ``processed`` as ``(first token, last token)``"""
    out, first = [], None
    for i, c in enumerate(processed):
        if c != ' ' and first is None:
            first = i
        if first is not None and (c == ' ' or i == len(processed) - 1):
            out.append((first, i - 1 if c == ' ' else i))
            first = None
    return out


def marks_of_row(processed, spans, start, r, hop, rate=1.0, n_held=None, rate_in=22050, rate_out=None, n_out=None, kind='word',
                 raw=None, stats=None, place=None, spoken=True, offset=0, place_end=None):
    """The marks of one row: a list of dicts, the 'sentence' mark first, then the words (``kind`` 'word') or the words and
    characters ('char') in the order they are spoken.

    ``processed`` / ``spans``: ``token_spans`` of the row's sentence -- token j is character j, token len(processed) the end
    token; ``start``: the row's ``start`` of tts_token_times; ``r``, ``hop``, ``rate``, ``n_held``: ``step_sample``; ``place``: what
    a position in the row becomes in the waveform the caller receives (``marks_of_text``; None: the row itself), at ``rate_in``;
    ``rate_out`` / ``n_out``: the rate and the length of what is delivered (None: ``rate_in``, the row's ``n_held``).  A word
    lasts from the start of its first token to the end of its last, the sentence from token 0 to the start of the end token.
    A mark: ``type``, ``time_ms`` and ``end_ms`` (float64, at the delivered rate's clock: 1000 * position / rate_in),
    ``sample`` and ``end_sample`` (``out_sample``), ``start`` and ``end`` (offsets into ``raw`` plus ``offset``), ``value``
    (``raw[start:end]``, or the processed characters where there is no raw text) and ``spoken``; the sentence mark also carries
    ``reliable`` where ``stats`` is given.  ``spoken`` False (a dropped, silent piece): every mark has zero length at ``place(0)``.
    ``place_end``: what the END of a mark goes through instead of ``place`` (None: ``place``) -- a map that jumps, as
    ``prosody.warp_position`` does across a pause, has two values at a border: where something ends and where the next thing starts."""
    n_tok = len(processed)
    if len(start) < n_tok + 1:
        raise ValueError('marks_of_row: {} tokens and the end token need {} start steps, got {}'.format(n_tok, n_tok + 1, len(start)))
    if n_held is None:
        raise ValueError('marks_of_row: n_held, the samples the row holds, is needed')
    rate_out = rate_in if rate_out is None else rate_out
    place = place or (lambda x: x)

    def position(j, through=None):
        return float((through or place)(step_sample(int(start[j]), r, hop, rate, n_held) if spoken else 0.0))

    limit = None if n_out is None else n_out

    def mark(kind_, a, b):            # tokens a .. b inclusive
        x0, x1 = position(a), position(b + 1, place_end)
        x1 = max(x1, x0)
        s0, e0 = (spans[a][0], spans[b][1]) if n_tok else (0, 0)
        n_lim = limit if limit is not None else out_sample(place(float(n_held)), rate_in, rate_out, float('inf'))
        return dict(type=kind_, time_ms=1000.0 * x0 / rate_in, end_ms=1000.0 * x1 / rate_in,
                    sample=out_sample(x0, rate_in, rate_out, n_lim), end_sample=out_sample(x1, rate_in, rate_out, n_lim),
                    start=offset + s0, end=offset + e0, value=raw[s0:e0] if raw is not None else processed[a:b + 1],
                    spoken=bool(spoken))

    out = []
    sentence = mark('sentence', 0, n_tok - 1) if n_tok else None
    if sentence is not None:
        if stats is not None:
            sentence['reliable'] = reliable(stats)
        out.append(sentence)
    for a, b in words_of(processed):
        out.append(mark('word', a, b))
        if kind == 'char':
            out += [mark('char', j, j) for j in range(a, b + 1)]
    return out


def join_offsets(pieces, groups):
    """o[p] of every piece of an ``Engine.join`` list ((P, 4) ``row, first, count, gap`` and the (P,) groups), by the layout rule
    of tts_join: 0 for a group's first piece, o[p + 1] = o[p] + count[p] + gap[p]"""
    o = np.zeros(len(pieces), dtype=np.int64)
    for p in range(1, len(pieces)):
        if groups[p] == groups[p - 1]:
            o[p] = o[p - 1] + int(pieces[p - 1][2]) + int(pieces[p - 1][3])
    return o


def marks_of_text(pieces, r, hop, rate=1.0, rate_in=22050, rate_out=None, n_out=None, kind='word', raw=None):
    """The marks of one text from those of its pieces, in the text's waveform.  ``pieces``: in order, one dict per piece with
    ``processed``, ``spans`` (``piece_spans``: offsets into ``raw``, the whole text), ``start`` (its row of
    tts_token_times), ``stats`` (or None) and, for a piece the join kept, ``n_held``, ``first``, ``count`` (its cut of the row),
    ``o`` (``join_offsets``) and ``part`` (where its call's part of the text starts in the text's waveform, as
    ``synthesize_text`` concatenates the parts); for a dropped, silent piece ``at``, the end of what was said before it.  A
    position x of a kept piece's row becomes ``clip(x - first, 0, count) + o + part``; a dropped piece gives zero-length marks
    with ``spoken`` False.  The sentence marks of the pieces stay, one per piece."""
    out = []
    for p in pieces:
        if 'at' in p:
            out += marks_of_row(p['processed'], p['spans'], p['start'], r, hop, rate, 0, rate_in, rate_out, n_out, kind,
                                raw=raw, stats=p.get('stats'), place=lambda x, p=p: float(p['at']), spoken=False)
        else:
            out += marks_of_row(p['processed'], p['spans'], p['start'], r, hop, rate, p['n_held'], rate_in, rate_out, n_out, kind,
                                raw=raw, stats=p.get('stats'),
                                place=lambda x, p=p: min(max(x - p['first'], 0.0), float(p['count'])) + p['o'] + p['part'])
    return out


def write_marks(path, marks):
    """the marks as JSON lines, one mark per line"""
    with open(path, 'w') as f:
        for m in marks:
            f.write(json.dumps(m) + '\n')
