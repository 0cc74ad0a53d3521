"""GPU: tts_alignment_stats and tts_text_lengths (csrc/alignment.hip) against the sequential numpy oracle of
tests/alignment_oracle.py, bit for bit: every integer of the record, the focus sum as a 64-bit pattern, the durations, the
positions and the bits of the weights there.

Shapes: the smallest at which the kernels can go wrong -- rows shorter than a wave, one element off a wave (63, 64, 65), the
reference's 92, rows beyond what a wave reaches in one 16-byte load each (257) and in several (1100); odd widths put the rows at
every offset from a 16-byte boundary; 1, 2 and 40 steps; one utterance and three; 65 utterances for the second launch's lengths."""
import ctypes

import numpy as np
import pytest

import alignment_cases as C
import alignment_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu


def run(engine, ali, n_sent=None, n_steps=None):
    return engine.alignment_stats(ali, n_sent=n_sent, n_steps=n_steps, want_durations=True, want_pos=True)


def assert_oracle(engine, ali, n_sent=None, n_steps=None, what=None):
    stats, dur, pos, peak = run(engine, ali, n_sent, n_steps)
    w_stats, w_dur, w_pos, w_peak = O.batch(ali, n_sent, n_steps)
    assert np.array_equal(pos, w_pos), what
    assert np.array_equal(peak.view(np.uint32), w_peak.view(np.uint32)), what
    assert np.array_equal(dur, w_dur), what
    assert O.same_records(stats, w_stats), (what, stats, w_stats)
    return stats


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S', [1, 2, 40])
@pytest.mark.parametrize('Ts', [1, 5, 63, 64, 65, 92, 257, 1100])
def test_the_record_is_the_oracle_bit_for_bit(engine, Ts, S, B):
    stats = assert_oracle(engine, C.random_batch(S, B, Ts), what=(Ts, S, B))
    assert np.all(stats['n_sent'] == Ts) and np.all(stats['n_steps'] == S) and np.all(stats['reserved'] == 0)
    assert np.all(np.isfinite(stats['focus_sum'])) and np.all(stats['focus_sum'] > 0)


def test_the_hand_written_cases(engine):
    ali, n_sent, n_steps, names = C.hand_batch()
    stats, dur, pos, _peak = run(engine, ali, n_sent, n_steps)
    for b, name in enumerate(names):
        rows, N, rec, w_dur, w_pos = C.HAND[name]
        for field, value in rec.items():
            got = stats[field][b]
            assert (np.isnan(got) and np.isnan(value)) or got == value, (name, field, got, value)
        assert list(dur[b, :rows.shape[1]]) == w_dur and not dur[b, rows.shape[1]:].any(), name
        assert list(pos[b, :rows.shape[0]]) == w_pos and np.all(pos[b, rows.shape[0]:] == -1), name


@pytest.mark.parametrize('S,B,Ts', [(40, 5, 92), (7, 4, 257), (3, 65, 65)])
def test_ragged_lengths_and_what_is_never_read(engine, S, B, Ts):
    """lengths of 1 and of the maximum among them; the steps behind an utterance's own are poisoned with NaN (never read), its
    padding columns hold real weights (read for off alone) -- and 65 utterances take a second launch's lengths"""
    ali = C.random_batch(S, B, Ts, tag=11)
    n_sent, n_steps = C.ragged_lengths(B, Ts, 1), C.ragged_lengths(B, S, 2)[::-1]
    assert {1, Ts} <= set(n_sent) and {1, S} <= set(n_steps)
    for b in range(B):
        ali[n_steps[b]:, b, :] = np.nan
    stats = assert_oracle(engine, ali, n_sent, n_steps, what=(S, B, Ts))
    assert list(stats['n_sent']) == n_sent and list(stats['n_steps']) == n_steps
    assert np.all(np.isfinite(stats['focus_sum']))          # no poisoned step reached a record
    if S * Ts > 1000:
        assert stats['off_text'].sum() > 0                  # ... and the padding was looked at
    # the padding decides off and nothing else: with other weights there, every other field stays
    other = ali.copy()
    for b in range(B):
        other[:, b, n_sent[b]:] = np.float32(2.0)
    again = assert_oracle(engine, other, n_sent, n_steps)
    for field in O.FIELDS + ('focus_sum',):
        if field != 'off_text':
            assert np.array_equal(again[field], stats[field]), field
    assert list(again['off_text']) == [n_steps[b] if n_sent[b] < Ts else 0 for b in range(B)]


def test_ties_at_the_lane_and_wave_reach_boundaries(engine):
    """the maximum twice: in neighbouring lanes of one load, across two lanes' float4s, across what a wave reaches in one load
    (64 lanes x 4 floats), and with the LOWER index in the later load -- the lower index wins every time"""
    Ts = 1100
    pairs = [(0, 1), (3, 4), (63, 64), (255, 256), (256, 257), (10, 300), (511, 512), (1023, 1099), (700, 2)]
    ali = np.full((len(pairs), 2, Ts), 0.25, np.float32) * C.random_batch(len(pairs), 2, Ts, tag=5)
    for s, (i, j) in enumerate(pairs):
        ali[s, :, i] = ali[s, :, j] = np.float32(0.5)
    ali[:, 1, :] = np.roll(ali[:, 1, :], 1, axis=1)         # utterance 1: the same one element on (another row alignment too)
    _stats, _dur, pos, peak = run(engine, ali)
    assert list(pos[0]) == [min(p) for p in pairs]
    assert list(pos[1]) == [min((i + 1) % Ts, (j + 1) % Ts) for i, j in pairs]
    assert np.all(peak == np.float32(0.5))
    assert_oracle(engine, ali)
    # -0.0 and +0.0 are equal: the first of them wins
    z = np.full((1, 1, 70), -1.0, np.float32)
    z[0, 0, 66], z[0, 0, 5] = 0.0, -0.0
    _s, _d, pos, peak = run(engine, z)
    assert pos[0, 0] == 5 and np.signbit(peak[0, 0])


def test_nan_and_inf(engine):
    S, Ts, N = 6, 92, 60
    base = C.random_batch(S, 1, Ts, tag=3)[:, 0]
    cases = {}
    for name, (where, value) in dict(nan_first=(0, np.nan), nan_last_of_text=(N - 1, np.nan), nan_in_padding=(N + 3, np.nan),
                                     nan_last=(Ts - 1, np.nan), inf_in_text=(17, np.inf), minus_inf=(17, -np.inf)).items():
        rows = base.copy()
        rows[2, where] = value
        cases[name] = rows
    two = base.copy()
    two[2, 40], two[2, 9], two[2, 70] = np.nan, np.nan, np.nan          # the first NaN of the text, and one in the padding
    cases['nan_twice'] = two
    both = base.copy()
    both[2, 30], both[2, 12] = np.inf, np.nan                            # a NaN beats +Inf
    cases['inf_and_nan'] = both
    names = list(cases)
    ali = np.ascontiguousarray(np.stack([cases[n] for n in names], axis=1))
    stats = assert_oracle(engine, ali, [N] * len(names))
    _s, _d, pos, peak = run(engine, ali, [N] * len(names))
    at = {n: (int(pos[b, 2]), peak[b, 2], stats[b]) for b, n in enumerate(names)}
    assert at['nan_first'][0] == 0 and np.isnan(at['nan_first'][1]) and np.isnan(at['nan_first'][2]['focus_sum'])
    assert at['nan_last_of_text'][0] == N - 1 and at['nan_last_of_text'][2]['end_step'] <= 2
    clean = O.utterance(base, N)[0]
    for name in ('nan_in_padding', 'nan_last'):                          # in the padding only: off, and nothing else
        rec = at[name][2]
        assert np.isfinite(rec['focus_sum']) and rec['focus_sum'] == clean['focus_sum'] and at[name][0] == O.utterance(base, N)[2][2]
        assert rec['off_text'] == clean['off_text'] + (0 if O.positions(base, N)[2][2] else 1)
    assert at['inf_in_text'][0] == 17 and np.isposinf(at['inf_in_text'][2]['focus_sum'])
    assert at['minus_inf'][0] != 17 and np.isfinite(at['minus_inf'][2]['focus_sum'])
    assert at['nan_twice'][0] == 9 and at['inf_and_nan'][0] == 12
    # a NaN in one utterance touches no other
    alone = engine.alignment_stats(np.ascontiguousarray(ali[:, names.index('minus_inf')][:, None]), n_sent=[N])
    assert O.same_records(alone, stats[names.index('minus_inf'):][:1])


@pytest.mark.parametrize('N', [92, 60])
def test_the_reference_fixture(engine, N):
    rows = C.fixture()
    stats = assert_oracle(engine, rows[:, None, :], [N])
    rec = stats[0]
    if N == 92:
        assert rec['end_step'] == 0 and rec['after_end'] == 142 and round(rec['focus_sum'] / 200, 4) == 0.0109
    else:
        assert rec['end_step'] == -1 and rec['off_text'] == 70 and rec['longest_stall'] == 96
    assert 'unfocused' in pkg('tacotron.attention_check').verdict(rec)


def test_a_record_does_not_depend_on_the_batch_or_the_place_in_it(engine):
    S, Ts = 40, 92
    utts = [C.random_utterance(S, Ts, tag=20 + b) for b in range(6)]
    n_sent, n_steps = [92, 60, 1, 17, 91, 33], [40, 1, 40, 13, 39, 2]
    ali = np.ascontiguousarray(np.stack(utts, axis=1))
    stats = assert_oracle(engine, ali, n_sent, n_steps)
    back = engine.alignment_stats(np.ascontiguousarray(ali[:, ::-1]), n_sent=n_sent[::-1], n_steps=n_steps[::-1])
    assert O.same_records(back[::-1], stats)
    for b in range(6):
        alone = engine.alignment_stats(np.ascontiguousarray(ali[:n_steps[b], b:b + 1]), n_sent=n_sent[b:b + 1])
        assert O.same_records(alone, stats[b:b + 1]), b
    # ... nor on the batch being cut into launches: 70 utterances, the six among them
    many = np.ascontiguousarray(np.stack([utts[b % 6] for b in range(70)], axis=1))
    big = engine.alignment_stats(many, n_sent=[n_sent[b % 6] for b in range(70)], n_steps=[n_steps[b % 6] for b in range(70)])
    for b in range(70):
        assert O.same_records(big[b:b + 1], stats[b % 6:b % 6 + 1]), b


def test_the_optional_outputs_and_their_null_forms(engine):
    ali = C.random_batch(9, 3, 65, tag=31)
    n_sent, n_steps = [65, 20, 1], [9, 4, 1]
    full = run(engine, ali, n_sent, n_steps)
    plain = engine.alignment_stats(ali, n_sent=n_sent, n_steps=n_steps)
    assert O.same_records(plain, full[0])
    stats, dur = engine.alignment_stats(ali, n_sent=n_sent, n_steps=n_steps, want_durations=True)
    assert O.same_records(stats, full[0]) and np.array_equal(dur, full[1])
    stats, pos, peak = engine.alignment_stats(ali, n_sent=n_sent, n_steps=n_steps, want_pos=True)
    assert O.same_records(stats, full[0]) and np.array_equal(pos, full[2]) and np.array_equal(peak.view(np.uint32), full[3].view(np.uint32))
    assert np.all(pos[1, 4:] == -1) and not peak[1, 4:].any() and np.all(dur.sum(axis=1) == n_steps)
    # a device buffer in, the same out
    d = engine.to_device(ali)
    try:
        assert O.same_records(engine.alignment_stats(d, n_sent=n_sent, n_steps=n_steps), full[0])
    finally:
        d.free()


def test_text_lengths(engine):
    ids = np.zeros((7, 70), np.int32)
    ids[1, :] = 5                                   # no padding
    ids[2, :23] = np.arange(1, 24)
    ids[3, 0] = 9
    ids[4, :40] = 3
    ids[4, 10:20] = 0                               # the pad id inside the sentence
    ids[5, 69] = 1
    ids[6, 64] = 2                                  # the last one in another lane's stride
    want = [1, 70, 23, 1, 40, 70, 65]
    assert list(O.text_lengths(ids)) == want
    assert list(engine.text_lengths(ids)) == want
    assert list(engine.text_lengths(ids, pad_id=3)) == list(O.text_lengths(ids, 3))
    assert list(engine.text_lengths(np.full((2, 1), 4, np.int32), pad_id=4)) == [1, 1]
    for Ts in (1, 63, 64, 65, 257):
        rng = np.random.default_rng(Ts)
        x = rng.integers(0, 3, (5, Ts)).astype(np.int32)
        assert list(engine.text_lengths(x)) == list(O.text_lengths(x)), Ts


def test_the_profile_stage_counts_two_launches_per_64_utterances(engine):
    engine.set_option('profile', 1)
    try:
        for B, launches in ((1, 2), (64, 2), (65, 4)):
            engine.profile_reset()
            engine.alignment_stats(C.random_batch(2, B, 5))
            assert engine.profile_get('alignment')[1] == launches, B
        engine.profile_reset()
        engine.text_lengths(np.zeros((3, 9), np.int32))
        assert engine.profile_get('alignment')[1] == 1
    finally:
        engine.set_option('profile', 0)


def test_the_library_refuses_bad_arguments(engine):
    H = pkg('_hip')
    lib, h, INV = engine.lib, engine.handle, H.TTS_ERR_INVALID
    d_ali = engine.to_device(C.random_batch(4, 3, 20))
    d_stats = engine.empty((3,), H.ALIGNMENT_RECORD)
    a, s = d_ali.data_ptr(), d_stats.data_ptr()

    def i32(values):
        return (ctypes.c_int32 * len(values))(*values)

    def why():
        return (lib.tts_last_error(h) or b'').decode()

    try:
        for args, text in (
                ((None, 4, 3, 20, None, None, s, None, None, None), 'alignment_stats: a NULL pointer (alignments and stats are required)'),
                ((a, 4, 3, 20, None, None, None, None, None, None), 'alignment_stats: a NULL pointer (alignments and stats are required)'),
                ((a, 0, 3, 20, None, None, s, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
                ((a, 4, 0, 20, None, None, s, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
                ((a, 4, 3, 0, None, None, s, None, None, None), 'alignment_stats: need B, Ts, n_steps_max >= 1'),
                ((a, 4, 3, 20, i32([20, 0, 5]), None, s, None, None, None), 'alignment_stats: n_sent[1] = 0 is not in 1 .. Ts = 20'),
                ((a, 4, 3, 20, i32([20, 1, 21]), None, s, None, None, None), 'alignment_stats: n_sent[2] = 21 is not in 1 .. Ts = 20'),
                ((a, 4, 3, 20, None, i32([5, 1, 1]), s, None, None, None), 'alignment_stats: n_steps[0] = 5 is not in 1 .. n_steps_max = 4'),
                ((a, 4, 3, 20, None, i32([4, -1, 1]), s, None, None, None), 'alignment_stats: n_steps[1] = -1 is not in 1 .. n_steps_max = 4'),
                ((a, 4, 3, 20, None, None, s + 4, None, None, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned'),
                ((a + 2, 4, 3, 20, None, None, s, None, None, None), 'alignment_stats: stats must be 8-byte aligned, the other buffers 4-byte aligned')):
            assert lib.tts_alignment_stats(h, *args) == INV and why() == text, (args, why())
        assert lib.tts_text_lengths(h, None, 3, 20, 0, s) == INV and why() == 'text_lengths: a NULL pointer (ids and n_sent are required)'
        assert lib.tts_text_lengths(h, a, 0, 20, 0, s) == INV and why() == 'text_lengths: need B, Ts >= 1'
        assert lib.tts_text_lengths(h, a, 3, 0, 0, s) == INV and why() == 'text_lengths: need B, Ts >= 1'
        # a refused call has enqueued nothing: the next good one is right
        assert lib.tts_alignment_stats(h, a, 4, 3, 20, None, None, s, None, None, None) == H.TTS_OK
        assert O.same_records(d_stats.to_host(), O.batch(d_ali.to_host())[0])
        # the fresh handle has no record of a synthesis call
        assert lib.tts_synth_alignment_stats(h, s, 3) == INV
    finally:
        d_ali.free()
        d_stats.free()
