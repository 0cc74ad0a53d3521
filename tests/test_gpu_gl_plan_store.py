"""GPU: the handle's store of Griffin-Lim run tables (csrc/api_internal.h, GlPlanStore) and the table of launch forms
(csrc/griffin_lim.hip, gl_stream_form).

The cut never decides a waveform's bits (test_gpu_audio.py::test_griffin_lim_bits_do_not_depend_on_the_cut) and the seed fixes
the start, so whatever the store has been through -- more cuts than it holds, tables overwritten and retired, another handle
destroyed, the stream changed -- a call returns the BITS of the same call on a fresh handle.  The shapes are the smallest that
take every path: T >= 7 is what 800 / 200 allows (hop (T - 1) > n_fft / 2), four iterations are a seeded first launch of three
iterations, a launch of one and the final iSTFT.  The launch forms are held to the oracles under the bounds of
test_gpu_audio.py, test_gpu_momentum.py and test_gpu_ragged_gl.py, through their helpers."""
import contextlib

import numpy as np
import pytest

import audio_cases as C
import momentum_oracle as M
import ragged_cases as R
from conftest import pkg, rel_l2
from oracle import audio_oracle as A
from parity import assert_segment_parity
from test_gpu_audio import seed_u
from test_gpu_ragged_gl import bits, check_against_oracle

pytestmark = pytest.mark.gpu

N_FFT, WIN, HOP = R.STREAM_800
N_ITER = 4
PLAN_CAPACITY = 16   # GL_PLAN_CAPACITY (csrc/api_internal.h)


@contextlib.contextmanager
def fresh_engine(hparams):
    eng = pkg().Engine(hparams)
    try:
        yield eng
    finally:
        eng.close()


def uniform_input(B, T):
    return C.power4_mag(np.random.default_rng([B, T]), (B, 1025, T))


def ragged_input(lengths):
    mag = np.zeros((len(lengths), 1025, max(lengths)), np.float32)
    for b, T in enumerate(lengths):
        mag[b, :, :T] = C.power4_mag(np.random.default_rng([b, T]), (1025, T))
    return mag


def call(eng, mag, n_frames=None, **options):
    """a seeded tts_griffin_lim / tts_griffin_lim_ragged at 800 / 200 with the mse -> the bits of (waveform, mse)"""
    try:
        for k in sorted(options, key=lambda k: k != 'debug_hooks'):
            eng.set_option(k, options[k])
        wav, mse = eng.griffin_lim(mag, N_ITER, WIN, HOP, N_FFT, seed=11, want_mse=True, n_frames=n_frames)
        return bits(wav.to_host()), bits(mse.to_host())
    finally:
        for k in sorted(options, key=lambda k: k == 'debug_hooks'):
            eng.set_option(k, 0)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def on_fresh_handle(hparams, mag, n_frames=None, **options):
    with fresh_engine(hparams) as eng:
        out = call(eng, mag, n_frames, **options)
    assert np.isfinite(out[0].view(np.float32)).all() and out[0].any()
    return out


def test_more_cuts_than_the_store_holds(hparams):
    """20 shapes and four length vectors on one handle -- more than the store's entries, so tables are overwritten with other
    cuts -- then one cut of more runs than any table has room for (the old table is retired, not freed under the launches that
    may read it), then the first three shapes again, whose cuts are long gone: every call has the bits of a fresh handle's."""
    rng = np.random.default_rng(16)
    shapes = list(range(8, 28))
    assert len(shapes) + 4 > PLAN_CAPACITY
    with fresh_engine(hparams) as eng:
        for k, T in enumerate(shapes):
            mag = uniform_input(2, T)
            assert same(call(eng, mag), on_fresh_handle(hparams, mag)), 'T = {}'.format(T)
            if k % 5 == 4:
                lengths = [int(v) for v in rng.integers(7, 28, 3)]
                mag = ragged_input(lengths)
                assert same(call(eng, mag, lengths), on_fresh_handle(hparams, mag, lengths)), 'lengths {}'.format(lengths)
        # 3 x 700 frames in runs of 8: 264 runs, more than a table of 256
        mag = uniform_input(3, 700)
        forced = dict(debug_hooks=1, gl_run_len=8)
        assert same(call(eng, mag, **forced), on_fresh_handle(hparams, mag, **forced))
        for T in shapes[:3]:
            mag = uniform_input(2, T)
            assert same(call(eng, mag), on_fresh_handle(hparams, mag)), 'T = {} again'.format(T)
        eng.synchronize()   # (the retired table is freed here)
        mag = uniform_input(2, shapes[-1])
        assert same(call(eng, mag), on_fresh_handle(hparams, mag))


def test_a_handles_tables_outlive_another_handle(hparams):
    """two handles run one shape; the first is destroyed; the second runs the shape again: its own first result, bit for bit"""
    mag = uniform_input(2, 9)
    with fresh_engine(hparams) as second:
        with fresh_engine(hparams) as first:
            a = call(first, mag)
            b = call(second, mag)
        assert same(a, b)
        assert same(call(second, mag), b)


def test_tables_follow_the_handle_to_another_stream(hparams):
    """a shape on the handle's own stream, the same shape and a new one on an adopted stream (a plain hipStream_t, what
    torch.cuda.current_stream().cuda_stream is: test_gpu_full_size.py adopts one the same way), both again on a stream of the
    handle's own: the bits of a fresh handle's calls"""
    import ctypes
    hip = ctypes.CDLL('libamdhip64.so')
    known, new = uniform_input(2, 10), uniform_input(2, 13)
    want_known, want_new = on_fresh_handle(hparams, known), on_fresh_handle(hparams, new)
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    try:
        with fresh_engine(hparams) as eng:
            assert same(call(eng, known), want_known)
            eng.set_stream(stream.value)
            assert same(call(eng, known), want_known)
            assert same(call(eng, new), want_new)
            eng.set_stream(None)
            assert same(call(eng, known), want_known)
            assert same(call(eng, new), want_new)
    finally:
        hip.hipStreamDestroy(stream)


# ---- the launch forms, one call each: (n_iter, with the mse, seeded start, momentum).  With the default three iterations per
# launch n_iter = 2, 3, 4 take the two- and three-iteration forms and the single one behind them; the mse is a launch of one
# iteration; a momentum call runs one iteration per launch: its first (seeded or not), a middle one and the one with the mse.
FORMS = ([(0, False, False, 0.0)] +
         [(1, mse, seeded, 0.0) for mse in (False, True) for seeded in (False, True)] +
         [(n, False, seeded, 0.0) for n in (2, 3, 4) for seeded in (False, True)] +
         [(3, mse, seeded, 0.99) for mse in (False, True) for seeded in (False, True)])
SEED = 5


@pytest.mark.parametrize('cfg', [R.STREAM, R.STREAM_800], ids=['1102-275', '800-200'])
def test_every_launch_form_uniform(engine, cfg):
    n_fft, win, hop = cfg
    B, T = 2, 8
    rng = np.random.default_rng(win)
    mag = C.synth_mag(rng, B, T, n_fft, hop, win)
    explicit = rng.random(mag.shape).astype(np.float32)
    drawn = seed_u(SEED, B, mag.shape[1], T)
    for n_iter, want_mse, seeded, momentum in FORMS:
        label = 'form {}/{} it={} mse={} seeded={} momentum={}'.format(win, hop, n_iter, want_mse, seeded, momentum)
        wav, mse = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=None if seeded else explicit, seed=SEED,
                                      want_mse=want_mse, momentum=momentum)
        wav, mse = wav.to_host(), (mse.to_host() if want_mse else None)
        for b in range(B):
            u = (drawn if seeded else explicit)[b]
            if momentum:
                ref_wav, ref_mse = M.griffin_lim_momentum(mag[b], win, hop, n_fft, n_iter, u, momentum)
            else:
                ref_wav, ref_mse = A.griffin_lim_v2(mag[b], win, hop, n_fft, n_iter, init_phase=u)
            e = rel_l2(wav[b], ref_wav)
            print('{} b={}: wav rel-L2 {:.3e} mse {} vs {}'.format(label, b, e, mse[b] if want_mse else None, ref_mse))
            assert wav[b].shape == ref_wav.shape
            assert e < C.gl_tol(n_iter)   # 1e-4 max(1, n_iter), seeded starts included (test_griffin_lim_seeded_start)
            if not seeded:                # explicit phases: every hop segment as well (gl_segments, _against_restatement)
                assert_segment_parity(wav[b], ref_wav, hop, C.gl_tol(n_iter), '{} b={}'.format(label, b))
            if want_mse:
                assert abs(mse[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9


@pytest.mark.parametrize('cfg', [R.STREAM, R.STREAM_800], ids=['1102-275', '800-200'])
def test_every_launch_form_ragged(engine, cfg):
    n_fft, win, hop = cfg
    lengths = [7, 8]
    mag, explicit = R.batch(cfg, lengths, fill=np.nan)
    drawn = seed_u(SEED, len(lengths), 1025, max(lengths))
    for n_iter, want_mse, seeded, momentum in FORMS:
        label = 'ragged form {}/{} it={} mse={} seeded={} momentum={}'.format(win, hop, n_iter, want_mse, seeded, momentum)
        wav, mse = engine.griffin_lim(mag, n_iter, win, hop, n_fft, init_phase=None if seeded else explicit, seed=SEED,
                                      want_mse=want_mse, momentum=momentum, n_frames=lengths)
        wav, mse = wav.to_host(), (mse.to_host() if want_mse else None)
        if not seeded:
            check_against_oracle(cfg, lengths, wav, mse, n_iter, want_mse, momentum=momentum, label=label)
            continue
        # as test_gpu_ragged_gl.py::test_seeded_start_draws_as_the_padded_layout_does holds a seeded ragged call to the oracle
        for b, T in enumerate(lengths):
            n = hop * (T - 1)
            ref_wav, ref_mse = R.reference(cfg, T, n_iter, momentum=momentum, init=drawn[b, :, :T], key=('seed', SEED, b, max(lengths)))
            e = rel_l2(wav[b, :n], ref_wav)
            print('{} b={}: wav rel-L2 {:.3e} mse {} vs {}'.format(label, b, e, mse[b] if want_mse else None, ref_mse))
            assert not wav[b, n:].any()
            assert e < 1e-4 * max(1, n_iter)
            if want_mse:
                assert abs(mse[b] - ref_mse) <= 1e-3 * abs(ref_mse) + 1e-9
