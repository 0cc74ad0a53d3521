"""CPU: the fast Griffin-Lim restatements of momentum_oracle.py, the fairness of the bounds test_gpu_momentum.py uses, the
convergence claim the option exists for, and the argument checks of the Python surface.

As in test_audio_bounds_host.py, a float32 restatement has to stay within a QUARTER of the bound the GPU test holds the
kernels to -- 1e-4 n_iter per hop segment, 1e-3 on the mse -- on exactly the inputs that test feeds them, so that a kernel
that keeps its momentum state in exact float32 has a fourfold margin.  (gl_second_window_input(2) is not among the cases:
float32 arithmetic alone is at 2.15e-4 there, above the quarter -- a power-4 spectrum full of near-zero bins.)
"""
import numpy as np
import pytest

import audio_cases as C
import momentum_oracle as M
from conftest import pkg
from oracle import audio_oracle as A
from parity import assert_segment_parity

QUARTER = C.HOST_MARGIN


@pytest.mark.parametrize('make,n_iter', [(lambda: C.gl_few_input(2, 12, 1), 1), (lambda: C.gl_per_launch_input(2, 40, 6), 6)],
                         ids=['few-2-12-1', 'per-launch-2-40-6'])
def test_momentum_zero_is_the_oracles_loop_bit_for_bit(make, n_iter):
    mag, init = make()
    for b in range(mag.shape[0]):
        ref_wav, ref_mse = A.griffin_lim_v2(mag[b], 1102, 275, 2048, n_iter, init_phase=init[b])
        wav, mse = M.griffin_lim_momentum(mag[b], 1102, 275, 2048, n_iter, init[b], momentum=0.0)
        assert wav.dtype == ref_wav.dtype and np.array_equal(wav.view(np.uint32), ref_wav.view(np.uint32))
        assert np.float64(mse).tobytes() == np.float64(ref_mse).tobytes()


def test_momentum_changes_the_result_from_the_second_iteration_on():
    """t_0 = c_0: one iteration is the plain one whatever alpha; two are not"""
    mag, init = C.gl_few_input(2, 12, 1)
    one = M.griffin_lim_momentum(mag[0], 1102, 275, 2048, 1, init[0], momentum=0.99)
    ref = A.griffin_lim_v2(mag[0], 1102, 275, 2048, 1, init_phase=init[0])
    assert np.array_equal(one[0], ref[0]) and one[1] == ref[1]
    two = M.griffin_lim_momentum(mag[0], 1102, 275, 2048, 2, init[0], momentum=0.99)
    ref2 = A.griffin_lim_v2(mag[0], 1102, 275, 2048, 2, init_phase=init[0])
    assert not np.array_equal(two[0], ref2[0])
    assert two[1] == ref2[1]   # the mse is that of the projection c_1, which the momentum has not touched yet


def _f32_check(key, case, label):
    mag, init, win, hop, n_fft, n_iter, momentum = case
    tol = QUARTER * C.gl_tol(n_iter)
    for b, (ref_wav, ref_mse) in enumerate(M.reference(key, case)):
        wav, mse = M.griffin_lim_momentum32(mag[b], win, hop, n_fft, n_iter, init[b], momentum)
        assert_segment_parity(wav, ref_wav, hop, tol, '{} b={}'.format(label, b))
        print('{} b={}: mse {} vs {}'.format(label, b, mse, ref_mse))
        assert abs(mse - ref_mse) <= QUARTER * 1e-3 * abs(ref_mse) + 1e-9


@pytest.mark.parametrize('momentum', [0.99, 0.5])
@pytest.mark.parametrize('k', range(len(C.GL_PER_LAUNCH)))
def test_float32_momentum_iterations_per_launch(k, momentum):
    _f32_check(('per_launch', k, momentum), M.case_per_launch(k, momentum),
               'f32 momentum {} per-launch {}'.format(momentum, C.GL_PER_LAUNCH[k]))


@pytest.mark.parametrize('per_launch', [1, 3])
def test_float32_momentum_second_window(per_launch):
    _f32_check(('second_window', per_launch), M.case_second_window(per_launch), 'f32 momentum 800/200 seed {}'.format(per_launch))


@pytest.mark.parametrize('k', range(5))
def test_float32_momentum_other_sizes(k):
    _f32_check(('other_sizes', k), M.case_other_sizes(k), 'f32 momentum {}'.format(C.GL_OTHER_SIZES[k]))


@pytest.mark.parametrize('run_len', [8, 104])
def test_float32_momentum_run_cut_inputs(run_len):
    _f32_check(('run_cut', run_len), M.case_run_cut(run_len), 'f32 momentum run-cut input {}'.format(run_len))


def test_momentum_reaches_the_plain_loops_quality_in_half_the_iterations():
    """What the option is for, on the reference's own spectrogram (frames 100:400): 30 iterations at alpha = 0.99 end with
    a lower mse than 60 plain ones (0.107 against 0.114 in spectral convergence, the square root of the mse up to a
    constant).  The one slow host test (about 20 s)."""
    mag, init = M.shipped_spectrogram()
    assert mag.shape == (1025, 300)
    fast, plain = [], []
    M.griffin_lim_momentum(mag, 1102, 275, 2048, 30, init, momentum=0.99, history=fast)
    M.griffin_lim_momentum(mag, 1102, 275, 2048, 60, init, momentum=0.0, history=plain)
    sc = lambda mse: np.sqrt(mse * mag.size) / np.linalg.norm(mag)   # noqa: E731
    print('spectral convergence: alpha 0.99 it 30 {:.4f}; alpha 0 it 30 {:.4f}, it 60 {:.4f}'.format(sc(fast[-1]), sc(plain[29]),
                                                                                                      sc(plain[-1])))
    assert fast[-1] < plain[-1]
    assert fast[-1] < plain[29]


# ---------------------------------------------------------------------------------------------- the Python surface
class _NoEngine(object):
    """stands where an Engine would: any use of it is the failure"""

    def __getattr__(self, name):
        raise AssertionError('the engine was touched ({})'.format(name))


class _NoModel(object):
    engine = _NoEngine()

    def __getattr__(self, name):
        raise AssertionError('the model was touched ({})'.format(name))


BAD = [-0.1, 1.0, float('nan')]


@pytest.mark.parametrize('momentum', BAD)
def test_audio_synthesis_refuses_a_momentum_outside_the_unit_interval(momentum):
    S = pkg('audio.synthesis')
    mag = np.ones((1025, 12), np.float32)
    with pytest.raises(ValueError):
        S.griffin_lim_v2(mag, 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), momentum=momentum)
    with pytest.raises(ValueError):
        S.spectrogram_to_wav(mag, 1102, 275, 2048, 2, seed=1, engine=_NoEngine(), momentum=momentum)


@pytest.mark.parametrize('momentum', BAD)
def test_tacotron_inference_and_serve_refuse_a_momentum_outside_the_unit_interval(momentum):
    I = pkg('tacotron.inference')
    ids = np.ones((1, 4), np.int32)
    with pytest.raises(ValueError):
        I.synthesize_batch(_NoModel(), ids, momentum=momentum)
    with pytest.raises(ValueError):
        next(I.synthesize_stream(_NoModel(), [ids], momentum=momentum))
    with pytest.raises(ValueError):
        next(I.inference_stream(_NoModel(), [ids], momentum=momentum))
    with pytest.raises(ValueError):
        I.synthesize_sentences(['a'], None, momentum=momentum)
    with pytest.raises(ValueError):
        I.main(['--momentum', repr(momentum)])
    V = pkg('tacotron.serve')
    with pytest.raises(ValueError):
        V.post_process_spectrograms(np.zeros((1, 5, 1025), np.float32), _NoEngine(), momentum=momentum)
    with pytest.raises(ValueError):
        next(V.serve(iter([['a']]), None, momentum=momentum))


def test_momentum_option_value_and_command_line():
    H = pkg('_hip')
    assert [H.momentum_thousandths(m) for m in (0, 0.0, 0.5, 0.9, 0.99, 0.999, 0.9999)] == [0, 0, 500, 900, 990, 999, 999]
    I = pkg('tacotron.inference')
    assert I.parse_args([]).momentum == 0.0
    assert I.parse_args(['--momentum', '0.99']).momentum == 0.99
    # what the library makes of the option is what the restatements use
    assert M.alpha_of(0.99) == np.float32(990 / 1000.0) and M.alpha_of(0.0) == 0
