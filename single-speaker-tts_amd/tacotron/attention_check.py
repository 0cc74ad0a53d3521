"""Attention diagnostics: did the decoder read the sentence?

``Engine.alignment_stats`` (tts_alignment_stats, include/sstts_hip.h) reduces an alignment history to one exact record per
utterance; this module turns a record into flags.  No reference counterpart -- the reference plots its alignments
(tacotron/model.py:552-598) and leaves the judgement to the eye.

The thresholds are UNTUNED HEURISTICS: no trained checkpoint exists in this repository to tune them on.  They are set far from
both a clean alignment (focus 0.5 .. 0.9, one token forward every step or two) and the failures they name, so that they flag what
is plainly broken; a deployment should set its own from alignments it trusts.
"""
import numpy as np

FLAGS = ('unfinished', 'unfocused', 'backward', 'skip', 'stall', 'off_text', 'wander')

MIN_FOCUS = 0.2          # mean weight at the attended token; a flat alignment over N tokens has 1 / N
MAX_BACK = 2             # tokens the attention may step back within the spoken part (a repeat goes back by a word)
MAX_JUMP = 4             # tokens it may jump ahead in one step (a skip drops a word)
MAX_STALL_STEPS = 30     # decoder steps it may rest on one token (1.5 s at 5 frames of 12.5 ms a step)
MAX_AFTER_END = 5        # steps behind the first visit of the last token that may leave it again


def _rows(stats):
    """the records as a list of dicts, and whether one record (not a batch) was given"""
    if isinstance(stats, dict):
        return [stats], True
    a = np.asarray(stats)
    if a.dtype.names is None:
        raise ValueError('verdict: records are needed (Engine.alignment_stats returns them), got an array of {}'.format(a.dtype))
    single = a.ndim == 0
    return [{name: r[name].item() for name in a.dtype.names} for r in a.reshape(-1)], single


def mean_focus(record):
    """focus_sum / n_steps: the mean weight at the attended token (NaN where a step's strongest weight was NaN)"""
    return float(record['focus_sum']) / float(record['n_steps'])


def verdict(stats, min_focus=MIN_FOCUS, max_back=MAX_BACK, max_jump=MAX_JUMP, max_stall_steps=MAX_STALL_STEPS,
            max_after_end=MAX_AFTER_END):
    """The flags of every utterance of ``stats`` -- the records of ``Engine.alignment_stats``, one record or a dict of its
    fields -- as a list of tuples (one tuple for one record); an empty tuple means clean.  Out of, in this order:

    ``unfinished``  the attention never stood on the last token (end_step == -1)
    ``unfocused``   the mean focus is below ``min_focus``, or is NaN
    ``backward``    it stepped back by more than ``max_back`` tokens within the spoken part
    ``skip``        it jumped ahead by more than ``max_jump`` tokens in one step, there
    ``stall``       it rested on one token for more than ``max_stall_steps`` steps, there
    ``off_text``    at some step the strongest weight of the whole padded row lay on padding
    ``wander``      more than ``max_after_end`` steps behind the first visit of the last token stood elsewhere

    The defaults are untuned heuristics (see the module)."""
    rows, single = _rows(stats)
    out = []
    for r in rows:
        focus = mean_focus(r)
        flags = []
        if r['end_step'] < 0:
            flags.append('unfinished')
        if not focus >= min_focus:
            flags.append('unfocused')
        if r['max_back'] > max_back:
            flags.append('backward')
        if r['max_jump'] > max_jump:
            flags.append('skip')
        if r['longest_stall'] > max_stall_steps:
            flags.append('stall')
        if r['off_text'] > 0:
            flags.append('off_text')
        if r['after_end'] > max_after_end:
            flags.append('wander')
        out.append(tuple(flags))
    return out[0] if single else out


def summary(record, flags=None):
    """one line for a person: the verdict and the numbers behind it"""
    rows, _single = _rows(record)
    r = rows[0]
    flags = verdict(r) if flags is None else tuple(flags)
    end = 'never' if r['end_step'] < 0 else 'step {}'.format(r['end_step'])
    return ('{}: {} tokens in {} steps, reached {} (last token: {}), focus {:.3f}, back {} x (max {}), jump {}, stall {}, '
            'skipped {}, off text {}, after end {}').format(
                'clean' if not flags else ' '.join(flags), r['n_sent'], r['n_steps'], r['reached'], end, mean_focus(r), r['backward'],
                r['max_back'], r['max_jump'], r['longest_stall'], r['skipped'], r['off_text'], r['after_end'])


def report(stats, **thresholds):
    """[{index, verdict, record}] of a batch of records: what ``--check-alignment`` prints, one JSON object per sentence"""
    rows, _single = _rows(stats)
    return [dict(index=i, verdict=list(verdict(r, **thresholds)), record=r) for i, r in enumerate(rows)]
