"""Cutting a text of any length into pieces the model can say (no reference counterpart: the reference synthesizes one line per
file and stops at ``max_iterations`` frames, tacotron/inference.py:139-143).

``split_text`` works on the raw text, before ``process_sentences``; ``tacotron.inference.synthesize_text`` turns the pieces into
ids, and the break behind every piece into the pause behind its waveform."""
import re

BREAKS = ('paragraph', 'sentence', 'clause', 'word', 'cut')
# 150 characters is the sentence length bench.py pairs with 200 decoder steps -- the one pairing of text length and step count the
# project measures -- not a tuned number.
MAX_CHARS = 150

_PARAGRAPH = re.compile(r'\n[^\S\n]*\n\s*')
_CLOSERS = '"\'”’)]}'
_SENTENCE_END = re.compile(r'[.!?]+[' + re.escape(_CLOSERS) + r']*(?= |$)')
_OPENERS = '"\'“‘([{'


def abbreviations_of(dataset):
    """the '.'-terminated keys of a dataset helper's ``_abbreviations`` ('mr.', 'dr.', ...; not the bare '.'), in lower case: what
    ``split_text`` does not end a sentence behind"""
    return tuple(sorted(k.lower() for k in getattr(dataset, '_abbreviations', {}) if k.endswith('.') and len(k) > 1))


def _sentences(par, abbreviations):
    """the sentences of a paragraph whose whitespace runs are single blanks already"""
    out, start = [], 0
    for m in _SENTENCE_END.finditer(par):
        if m.end() == len(par):
            break
        run = m.group().rstrip(_CLOSERS)
        if run == '.':
            word = par[par.rfind(' ', 0, m.start()) + 1:m.start() + 1].lstrip(_OPENERS).lower()
            # behind an abbreviation, or behind a single letter (an initial, 'J. S. Bach'): no end.  A '.' inside a number
            # ('3.14') has no blank behind it and is not looked at.
            if word in abbreviations or (len(word) == 2 and word[0].isalpha()):
                continue
        out.append(par[start:m.end()])
        start = m.end() + 1
    out.append(par[start:])
    return out


def _cut(sentence, max_chars):
    """a sentence as pieces of at most max_chars characters: ``[(piece, break), ...]``, the last break None"""
    out = []
    while len(sentence) > max_chars:
        head = sentence[:max_chars + 1]   # (a blank at max_chars leaves a piece of max_chars characters in front of it)
        clause = max((i for i in range(1, len(head)) if head[i] == ' ' and (head[i - 1] in ';:,' or head[i - 2:i] == ' -')), default=-1)
        blank = head.rfind(' ')
        if clause > 0:
            out.append((sentence[:clause], 'clause'))
            sentence = sentence[clause + 1:]
        elif blank > 0:
            out.append((sentence[:blank], 'word'))
            sentence = sentence[blank + 1:]
        else:
            out.append((sentence[:max_chars], 'cut'))
            sentence = sentence[max_chars:]
    out.append((sentence, None))
    return out


def split_text(text, max_chars=MAX_CHARS, abbreviations=()):
    """``text`` as a list of ``(piece, break)``: pieces of 1 .. ``max_chars`` characters and the break BEHIND each, one of
    'paragraph', 'sentence', 'clause', 'word', 'cut'.  Deterministic; the text is not changed but for its whitespace.

    Paragraphs end at blank lines (and at the end of the text).  Inside a paragraph every whitespace run counts as one blank.  A
    sentence ends behind a run of ``.!?`` and the closing quotes or brackets that follow it, where a blank or the end of the
    paragraph comes next -- but not behind one of ``abbreviations`` ('.'-terminated, compared in lower case: ``abbreviations_of``
    a dataset helper), not behind a single letter ('J. S. Bach'), and not inside a number ('3.14' has no blank behind its '.').
    A sentence longer than ``max_chars`` is cut at the last blank behind ``;``, ``:``, ``,`` or `` -`` that leaves at most
    ``max_chars`` characters in front of it ('clause'), failing that at the last such blank of any kind ('word'), failing that
    hard at ``max_chars`` characters ('cut'); the rest is cut the same way.

    The pieces, joined by one blank behind every break but 'cut' and by nothing behind a 'cut', are the text's paragraphs with
    their whitespace runs collapsed, joined by one blank.  ``max_chars`` defaults to 150, the sentence length bench.py pairs
    with 200 decoder steps: not a tuned number.  ValueError: ``max_chars`` < 1 or not an integer, ``text`` not a string."""
    if not isinstance(text, str):
        raise ValueError('split_text: text must be a string, got {!r}'.format(type(text).__name__))
    if isinstance(max_chars, bool) or not isinstance(max_chars, int) or max_chars < 1:
        raise ValueError('split_text: max_chars must be an integer >= 1, got {!r}'.format(max_chars))
    abbreviations = frozenset(a.lower() for a in abbreviations)
    out = []
    for par in _PARAGRAPH.split(text):
        par = ' '.join(par.split())
        if not par:
            continue
        for sentence in _sentences(par, abbreviations):
            for piece, brk in _cut(sentence, max_chars):
                out.append((piece, brk or 'sentence'))
        out[-1] = (out[-1][0], 'paragraph')
    return out


def split_text_spans(text, max_chars=MAX_CHARS, abbreviations=()):
    """``split_text`` with the place of every piece in the raw text: a list of ``(piece, break, start, end)`` whose first two
    fields are ``split_text``'s output, and ``text[start:end]`` with its whitespace runs collapsed is the piece.  The pieces lie
    in the text in order and do not overlap; what lies between them is whitespace."""
    out, at = [], 0
    for piece, brk in split_text(text, max_chars, abbreviations):
        while text[at].isspace():
            at += 1
        start = at
        for c in piece:
            if c == ' ':                      # one blank of a piece is a whitespace run of the text
                while text[at].isspace():
                    at += 1
            else:
                assert text[at] == c, (piece, at)
                at += 1
        out.append((piece, brk, start, at))
    return out
