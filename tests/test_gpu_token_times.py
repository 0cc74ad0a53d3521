"""GPU: tts_token_times (csrc/token_times.hip) against the sequential numpy oracle of tests/marks_oracle.py, bit for bit: start,
the path and every integer of the record.

Shapes (marks_cases.SHAPES): the smallest at which the kernel can go wrong -- one step and two, steps and columns one off a wave
(63, 64, 65), 130, columns beyond the 256 one pass of the lanes covers (300); directions in LDS (130 x 130) and in the workspace
(130 x 300); one utterance, three, and 65 for the second launch's lengths; the shortest, a short and the longest jump."""
import ctypes

import numpy as np
import pytest

import marks_cases as C
import marks_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu


def assert_oracle(engine, ali, n_sent=None, n_steps=None, J=4, what=None):
    start, stats, path = engine.token_times(ali, n_sent=n_sent, n_steps=n_steps, max_jump=J, want_path=True)
    w_start, w_stats, w_path = O.batch(ali, n_sent, n_steps, J)
    assert np.array_equal(path, w_path), what
    assert np.array_equal(start, w_start), what
    assert O.same_records(stats, w_stats), (what, stats, w_stats)
    return start, stats, path


@pytest.mark.parametrize('kind', ['mixed', 'staircase', 'special'])
@pytest.mark.parametrize('S,B,Ts,J', C.SHAPES)
def test_the_result_is_the_oracle_bit_for_bit(engine, S, B, Ts, J, kind):
    start, stats, path = assert_oracle(engine, C.batch(kind, S, B, Ts), J=J, what=(S, B, Ts, J, kind))
    assert np.all(stats['n_sent'] == Ts) and np.all(stats['n_steps'] == S)
    assert np.all(start[:, 0] == 0) and np.all(np.diff(start, axis=1) >= 0) and np.all(start[:, -1] == S)
    assert np.all(np.diff(path, axis=1) >= 0) and np.all(np.diff(path, axis=1) <= J) and np.all(path[:, 0] <= J)


def test_the_planted_staircase_comes_back(engine):
    rng = np.random.default_rng(0)
    m = C.STAIRCASE
    made = [C.staircase(rng) for _ in range(8)]
    ali = np.ascontiguousarray(np.stack([rows for rows, _t in made], axis=1))
    _start, stats, path = assert_oracle(engine, ali, J=m['J'])
    for b, (_rows, true) in enumerate(made):
        assert np.array_equal(path[b], true), b
    assert np.all(stats['agree'] == m['S'] - 4)          # the four outlier rows are where the argmax stands elsewhere


def test_the_tie_rules(engine):
    """all-equal rows: every path ties -- the smallest d everywhere and the lowest last column keep the path on token 0; all-zero
    rows the same with a score of 0"""
    for value, S, Ts in ((0.25, 9, 70), (0.0, 9, 70), (0.25, 3, 300)):
        ali = np.full((S, 2, Ts), value, np.float32)
        start, stats, path = assert_oracle(engine, ali, J=2)
        assert not path.any() and np.all(start[:, 1:] == S) and np.all(stats['last'] == 0) and np.all(stats['skipped'] == 0)
        assert np.all(stats['score'] == S * int(np.float32(value).view(np.uint32)))


@pytest.mark.parametrize('S,B,Ts,J', [(40, 5, 92, 4), (130, 4, 300, 2), (3, 65, 65, 15)])
def test_ragged_lengths_and_what_is_never_read(engine, S, B, Ts, J):
    """lengths of 1 and of the maximum among them; the columns at or behind an utterance's sentence and the steps at or behind its
    own are poisoned with NaN, then with large weights: nothing changes"""
    ali = C.batch('mixed', S, B, Ts, tag=11)
    n_sent, n_steps = C.ragged_lengths(B, Ts, 1), C.ragged_lengths(B, S, 2)[::-1]
    assert {1, Ts} <= set(n_sent) and {1, S} <= set(n_steps)
    clean = assert_oracle(engine, ali, n_sent, n_steps, J, what=(S, B, Ts))
    assert list(clean[1]['n_sent']) == n_sent and list(clean[1]['n_steps']) == n_steps
    for poison in (np.nan, 3e38):
        other = ali.copy()
        for b in range(B):
            other[n_steps[b]:, b, :] = poison
            other[:, b, n_sent[b]:] = poison
        got = engine.token_times(other, n_sent=n_sent, n_steps=n_steps, max_jump=J, want_path=True)
        assert np.array_equal(got[0], clean[0]) and O.same_records(got[1], clean[1]) and np.array_equal(got[2], clean[2])
    for b in range(B):                                      # behind the sentence start holds S, behind the steps the path -1
        assert np.all(clean[0][b, n_sent[b] + 1:] == n_steps[b]) and np.all(clean[2][b, n_steps[b]:] == -1)


class Shifted(object):
    """a device buffer seen `floats` elements behind its start"""

    def __init__(self, buf, floats, shape):
        self.buf, self.floats, self.shape = buf, floats, shape

    def data_ptr(self):
        return self.buf.data_ptr() + 4 * self.floats


@pytest.mark.parametrize('Ts', [65, 300])
def test_the_base_pointer_off_a_16_byte_boundary(engine, Ts):
    S, B = 7, 3
    ali = C.batch('special', S, B, Ts, tag=5)
    want = O.batch(ali, None, None, 3)
    room = engine.empty((ali.size + 4,), np.float32)
    try:
        assert room.data_ptr() % 16 == 0
        for off in (1, 2, 3):
            flat = np.zeros(ali.size + 4, np.float32)
            flat[off:off + ali.size] = ali.ravel()
            room.copy_from(flat)
            got = engine.token_times(Shifted(room, off, ali.shape), max_jump=3, want_path=True)
            assert np.array_equal(got[0], want[0]) and O.same_records(got[1], want[1]) and np.array_equal(got[2], want[2]), off
    finally:
        room.free()


def test_special_values(engine):
    """a NaN, a zero of either sign and a negative weigh nothing; +Inf and a denormal weigh their bits"""
    S, Ts = 4, 6
    rows = np.full((S, Ts), 0.125, np.float32)
    cases = {}
    for name, value in dict(nan=np.nan, inf=np.inf, minus_inf=-np.inf, minus_zero=-0.0, negative=-1.0, denormal=1e-45).items():
        r = rows.copy()
        r[:, 0] = value                                      # the whole of token 0
        cases[name] = r
    names = list(cases)
    ali = np.ascontiguousarray(np.stack([cases[n] for n in names], axis=1))
    _start, stats, path = assert_oracle(engine, ali, J=1)
    at = {n: (stats[b], path[b]) for b, n in enumerate(names)}
    one = int(np.float32(0.125).view(np.uint32))
    assert at['inf'][0]['score'] == S * 0x7f800000 and not at['inf'][1].any()
    for name in ('nan', 'minus_inf', 'minus_zero', 'negative', 'denormal'):
        assert at[name][0]['score'] == S * one and list(at[name][1]) == [1, 1, 1, 1], name
    # a NaN in one utterance touches no other
    b = names.index('denormal')
    alone = engine.token_times(np.ascontiguousarray(ali[:, b:b + 1]), max_jump=1)
    assert O.same_records(alone[1], stats[b:b + 1])


def test_a_result_does_not_depend_on_the_batch_or_the_place_in_it(engine):
    S, Ts, J = 40, 92, 4
    utts = [C.utterance(C.KINDS[b % 5], S, Ts, tag=20 + b) for b in range(6)]
    n_sent, n_steps = [92, 60, 1, 17, 91, 33], [40, 1, 40, 13, 39, 2]
    ali = np.ascontiguousarray(np.stack(utts, axis=1))
    start, stats, path = assert_oracle(engine, ali, n_sent, n_steps, J)
    for b in range(6):                                       # every utterance is its own B = 1 call
        one = engine.token_times(np.ascontiguousarray(ali[:n_steps[b], b:b + 1]), n_sent=n_sent[b:b + 1], max_jump=J, want_path=True)
        assert np.array_equal(one[0], start[b:b + 1]) and O.same_records(one[1], stats[b:b + 1]), b
        assert np.array_equal(one[2][0], path[b, :n_steps[b]]), b
    # ... nor on the batch being cut into launches: 70 utterances, the six among them
    many = np.ascontiguousarray(np.stack([utts[b % 6] for b in range(70)], axis=1))
    big = engine.token_times(many, n_sent=[n_sent[b % 6] for b in range(70)], n_steps=[n_steps[b % 6] for b in range(70)], max_jump=J)
    for b in range(70):
        assert np.array_equal(big[0][b], start[b % 6]) and O.same_records(big[1][b:b + 1], stats[b % 6:b % 6 + 1]), b


@pytest.mark.parametrize('S,Ts', [(9, 65), (130, 300)])
def test_without_a_path_start_is_the_same(engine, S, Ts):
    ali = C.batch('mixed', S, 3, Ts, tag=31)
    n_sent, n_steps = [Ts, 20, 1], [S, 4, 1]
    full = engine.token_times(ali, n_sent=n_sent, n_steps=n_steps, want_path=True)
    plain = engine.token_times(ali, n_sent=n_sent, n_steps=n_steps)
    assert len(plain) == 2 and np.array_equal(plain[0], full[0]) and O.same_records(plain[1], full[1])
    d = engine.to_device(ali)                               # a device buffer in, the same out
    try:
        again = engine.token_times(d, n_sent=n_sent, n_steps=n_steps)
        assert np.array_equal(again[0], full[0]) and O.same_records(again[1], full[1])
    finally:
        d.free()


def test_the_reference_fixture(engine):
    rows = C.fixture()
    _start, stats, path = assert_oracle(engine, rows[:, None, :], [92])
    assert np.all(np.diff(path[0]) >= 0) and not O.reliable(stats[0])


def test_the_profile_stage_counts_two_launches_per_64_utterances(engine):
    engine.set_option('profile', 1)
    try:
        for B, launches in ((1, 2), (64, 2), (65, 4)):
            engine.profile_reset()
            engine.token_times(C.batch('uniform', 2, B, 5))
            assert engine.profile_get('alignment')[1] == launches, B
    finally:
        engine.set_option('profile', 0)


def test_the_library_refuses_bad_arguments(engine):
    H = pkg('_hip')
    lib, h, INV, UNS = engine.lib, engine.handle, H.TTS_ERR_INVALID, H.TTS_ERR_UNSUPPORTED
    ali = C.batch('uniform', 4, 3, 20)
    d_ali = engine.to_device(ali)
    d_start = engine.empty((3, 21), np.int32)
    d_stats = engine.empty((3,), H.TOKEN_TIMES_RECORD)
    a, st, s = d_ali.data_ptr(), d_start.data_ptr(), d_stats.data_ptr()

    def i32(values):
        return (ctypes.c_int32 * len(values))(*values)

    def why():
        return (lib.tts_last_error(h) or b'').decode()

    try:
        for args, code, text in (
                ((None, 4, 3, 20, None, None, 4, st, None, s), INV, 'token_times: a NULL pointer (alignments, start and stats are required)'),
                ((a, 4, 3, 20, None, None, 4, None, None, s), INV, 'token_times: a NULL pointer (alignments, start and stats are required)'),
                ((a, 4, 3, 20, None, None, 4, st, None, None), INV, 'token_times: a NULL pointer (alignments, start and stats are required)'),
                ((a, 0, 3, 20, None, None, 4, st, None, s), INV, 'token_times: need B, Ts, n_steps_max >= 1'),
                ((a, 4, 3, 20, i32([20, 0, 5]), None, 4, st, None, s), INV, 'token_times: n_sent[1] = 0 is not in 1 .. Ts = 20'),
                ((a, 4, 3, 20, None, i32([5, 1, 1]), 4, st, None, s), INV, 'token_times: n_steps[0] = 5 is not in 1 .. n_steps_max = 4'),
                ((a, 4, 3, 20, None, None, 0, st, None, s), INV, 'token_times: max_jump = 0 is not in 1 .. 15'),
                ((a, 4, 3, 20, None, None, 16, st, None, s), INV, 'token_times: max_jump = 16 is not in 1 .. 15'),
                ((a, 4, 3, 20, None, None, 4, st, None, s + 4), INV, 'token_times: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
                ((a + 2, 4, 3, 20, None, None, 4, st, None, s), INV, 'token_times: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
                ((a, 4, 3, 1025, None, None, 4, st, None, s), UNS, 'token_times: Ts = 1025 is above the 1024 tokens of a table')):
            assert lib.tts_token_times(h, *args) == code and why() == text, (args, why())
        assert lib.tts_token_times_max_tokens() == H.TOKEN_TIMES_MAX_TOKENS >= 1024
        # a refused call has enqueued nothing: the next good one is right
        assert lib.tts_token_times(h, a, 4, 3, 20, None, None, 4, st, None, s) == H.TTS_OK
        w_start, w_stats, _p = O.batch(ali, None, None, 4)
        assert np.array_equal(d_start.to_host(), w_start) and O.same_records(d_stats.to_host(), w_stats)
    finally:
        for d in (d_ali, d_start, d_stats):
            d.free()
