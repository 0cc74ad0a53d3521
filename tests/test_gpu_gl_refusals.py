"""GPU: what tts_griffin_lim, tts_griffin_lim_ragged, tts_stft and tts_stft_magnitude answer to arguments they refuse -- the
return code and the text of tts_last_error, literally, through the C entry points themselves (the Python wrappers check most
of this first).  The rules are stated once (gl_refusal, csrc/gl_plan.h; tests/gl_rules_check.cpp holds the function itself to
the same texts); the entry points ask them in different orders and under different names, and where a call breaks several
rules the first one in the entry point's own order answers.

Buffers: B = 2, F = 1025 (n_fft 2048) or 129 (n_fft 256), T = 12.  A refused call enqueues and prepares nothing that a later
call could see: after the last refusal one legal call per entry point and kernel family gives the bits a fresh handle gives."""
import ctypes

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
B, T = 2, 12

NFFT = 'n_fft must be a power of two between 256 and 4096'
WINDOW_T = 'griffin_lim: need 2 <= win_length <= n_fft, hop_length >= 1, T >= 1'
SHORT = 'signal shorter than n_fft/2 (reflect padding undefined)'

# tts_griffin_lim: (n_fft, win, hop, T, B, n_iter) -> code, text
GL_CASES = [
    ((2048, 1102, 275, T, 0, 1), INVALID, 'griffin_lim: bad arguments'),
    ((2048, 1102, 275, T, B, -1), INVALID, 'griffin_lim: bad arguments'),
    ((250, 200, 50, T, B, 1), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((128, 100, 25, T, B, 1), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((8192, 1102, 275, T, B, 1), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((2048, 1, 275, T, B, 1), INVALID, WINDOW_T),
    ((2048, 2049, 275, T, B, 1), INVALID, WINDOW_T),
    ((2048, 1102, 0, T, B, 1), INVALID, WINDOW_T),
    ((2048, 1102, 275, 0, B, 1), INVALID, WINDOW_T),          # the streaming kernel's pair
    ((2048, 1000, 250, 0, B, 1), INVALID, WINDOW_T),          # the general kernels
    ((256, 200, 50, 0, B, 1), INVALID, WINDOW_T),
    ((2048, 512, 128, 9, B, 1), INVALID, 'griffin_lim: ' + SHORT),    # hop (T - 1) == n_fft / 2
    ((256, 64, 16, 9, B, 1), INVALID, 'griffin_lim: ' + SHORT),       # likewise
    ((2048, 1102, 275, 4, B, 1), INVALID, 'griffin_lim: ' + SHORT),   # the streaming kernel's pair: 825 <= 1024
    ((2048, 800, 200, 6, B, 1), INVALID, 'griffin_lim: ' + SHORT),
    # two rules at once: the first in the entry point's order answers
    ((2048, 1102, 275, 0, 0, 1), INVALID, 'griffin_lim: bad arguments'),
    ((250, 1, 50, T, B, 1), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((8192, 1102, 0, 0, B, 1), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((2048, 1, 128, 9, B, 1), INVALID, WINDOW_T),
    ((256, 257, 16, 9, B, 1), INVALID, WINDOW_T),
]

# tts_griffin_lim_ragged: (n_fft, win, hop, T_max, n_frames or None) -> code, text
RAGGED = 'griffin_lim_ragged: '
RAGGED_CASES = [
    ((2048, 1102, 275, T, None), INVALID, RAGGED + 'bad arguments'),
    ((250, 200, 50, T, [12, 9]), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((128, 100, 25, T, [12, 9]), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((8192, 1102, 275, T, [12, 9]), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((2048, 1, 275, T, [12, 9]), INVALID, WINDOW_T),
    ((2048, 2049, 275, T, [12, 9]), INVALID, WINDOW_T),
    ((2048, 1102, 0, T, [12, 9]), INVALID, WINDOW_T),
    ((2048, 1102, 275, 0, [12, 9]), INVALID, WINDOW_T),
    ((256, 200, 50, 0, [12, 9]), INVALID, WINDOW_T),
    ((2048, 1102, 275, T, [12, 0]), INVALID, RAGGED + 'n_frames[1] = 0 is not in 1 .. T_max = 12'),
    ((2048, 1102, 275, T, [12, 13]), INVALID, RAGGED + 'n_frames[1] = 13 is not in 1 .. T_max = 12'),
    ((2048, 1102, 275, T, [12, 4]), INVALID, RAGGED + 'utterance 1 (4 frames): ' + SHORT),
    ((256, 64, 16, T, [12, 9]), INVALID, RAGGED + 'utterance 1 (9 frames): ' + SHORT),      # hop (n - 1) == n_fft / 2
    ((256, 200, 50, T, [13, 9]), INVALID, RAGGED + 'n_frames[0] = 13 is not in 1 .. T_max = 12'),
    # two rules at once
    ((250, 1, 50, T, [12, 0]), UNSUPPORTED, 'griffin_lim: ' + NFFT),
    ((2048, 1, 275, T, [12, 0]), INVALID, WINDOW_T),
    ((2048, 1102, 275, 0, [0, 0]), INVALID, WINDOW_T),
    ((2048, 1102, 275, T, [4, 0]), INVALID, RAGGED + 'utterance 0 (4 frames): ' + SHORT),   # utterance by utterance
    ((2048, 1102, 275, T, [0, 4]), INVALID, RAGGED + 'n_frames[0] = 0 is not in 1 .. T_max = 12'),
    ((2048, 1102, 275, T, [13, 4]), INVALID, RAGGED + 'n_frames[0] = 13 is not in 1 .. T_max = 12'),
]

# tts_stft / tts_stft_magnitude: (n_fft, win, hop, n, B) -> code, text ({} = the entry point's name).  n_fft 2048 asks the window
# first and the general kernels' sizes the signal first; the general kernels' table rules carry no name.
STFT_WINDOW, GENERAL_WINDOW = 'stft: need 2 <= win_length <= n_fft, hop >= 1', 'need 2 <= win_length <= n_fft, hop_length >= 1'
N = 275 * (T - 1)
STFT_CASES = [
    ((2048, 1102, 275, N, 0), INVALID, '{}: bad arguments'),
    ((2048, 1, 275, N, B), INVALID, STFT_WINDOW),
    ((2048, 2049, 275, N, B), INVALID, STFT_WINDOW),
    ((2048, 1102, 0, N, B), INVALID, STFT_WINDOW),
    ((2048, 1102, 275, 1024, B), INVALID, 'stft: ' + SHORT),
    ((2048, 1102, 275, 0, B), INVALID, 'stft: ' + SHORT),
    ((250, 200, 50, N, B), UNSUPPORTED, NFFT),
    ((128, 100, 25, N, B), UNSUPPORTED, NFFT),
    ((8192, 1102, 275, 4097, B), UNSUPPORTED, NFFT),
    ((256, 1, 50, N, B), INVALID, GENERAL_WINDOW),
    ((256, 257, 50, N, B), INVALID, GENERAL_WINDOW),
    ((256, 200, 0, N, B), INVALID, GENERAL_WINDOW),
    ((256, 200, 50, 128, B), INVALID, 'stft: ' + SHORT),
    # two rules at once
    ((2048, 1, 0, 1024, 0), INVALID, '{}: bad arguments'),
    ((2048, 1, 275, 1024, B), INVALID, STFT_WINDOW),
    ((8192, 1102, 275, N, B), INVALID, 'stft: ' + SHORT),
    ((256, 1, 50, 128, B), INVALID, 'stft: ' + SHORT),
    ((250, 1, 0, N, B), UNSUPPORTED, NFFT),
]


def _last_error(eng):
    return (eng.lib.tts_last_error(eng.handle) or b'').decode()


def _legal_calls(eng, mag_h, mag129_h, sig_h):
    """one legal call per entry point and kernel family, 1 iteration; every result on the host"""
    out = []
    mag, mag129, sig = [eng.to_device(a) for a in (mag_h, mag129_h, sig_h)]
    for m, (n_fft, win, hop) in [(mag, (2048, 1102, 275)), (mag129, (256, 200, 50))]:
        for n_frames in (None, [12, 9]):
            wav, mse = eng.griffin_lim(m, 1, win, hop, n_fft, seed=5, n_frames=n_frames)
            out += [wav.to_host().copy(), mse.to_host().copy()]
            wav.free()
            mse.free()
        for f in (eng.stft, eng.stft_magnitude):
            o = f(sig, n_fft, win, hop)
            out.append(o.to_host().copy())
            o.free()
    for a in (mag, mag129, sig):
        a.free()
    return out


def test_refusals_are_the_literal_codes_and_texts(hparams):
    E = pkg().Engine
    used, fresh = E(hparams), E(hparams)
    rng = np.random.default_rng(2)
    mag_h, mag129_h = [rng.random((B, F, T), dtype=np.float32) + 0.1 for F in (1025, 129)]
    sig_h = rng.standard_normal((B, N)).astype(np.float32)
    try:
        lib, h = used.lib, used.handle
        mag, mag129 = used.to_device(mag_h), used.to_device(mag129_h)
        sig = used.to_device(np.zeros((B, 4400), np.float32))   # (room for the n = 4097 a refused call names)
        wav, spec = used.empty((B, N)), used.empty((B, 1025, T), np.complex64)
        seen = []
        for (n_fft, win, hop, t, b, n_iter), code, text in GL_CASES:
            m = mag129 if n_fft == 256 else mag
            rc = lib.tts_griffin_lim(h, m.data_ptr(), None, 0, b, t, n_iter, win, hop, n_fft, wav.data_ptr(), None)
            seen.append((('tts_griffin_lim', n_fft, win, hop, t, b, n_iter), (rc, _last_error(used)), (code, text)))
        for (n_fft, win, hop, t, lens), code, text in RAGGED_CASES:
            m = mag129 if n_fft == 256 else mag
            nf = np.array(lens, np.int32) if lens else None
            p = nf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if lens else None
            rc = lib.tts_griffin_lim_ragged(h, m.data_ptr(), None, 0, B, t, p, 1, win, hop, n_fft, wav.data_ptr(), None)
            seen.append((('tts_griffin_lim_ragged', n_fft, win, hop, t, lens), (rc, _last_error(used)), (code, text)))
        for name in ('stft', 'stft_magnitude'):
            for (n_fft, win, hop, n, b), code, text in STFT_CASES:
                args = (h, sig.data_ptr(), b, n, n_fft, win, hop) + ((1.0,) if name == 'stft_magnitude' else ()) + (spec.data_ptr(),)
                rc = getattr(lib, 'tts_' + name)(*args)
                seen.append((('tts_' + name, n_fft, win, hop, n, b), (rc, _last_error(used)), (code, text.format(name))))
        wrong = [s for s in seen if s[1] != s[2]]
        for s in wrong:
            print('%r answered %r, expected %r' % s)
        assert not wrong and len(seen) == len(GL_CASES) + len(RAGGED_CASES) + 2 * len(STFT_CASES)
        for a in (mag, mag129, sig, wav, spec):
            a.free()
        # nothing of the refused calls is left on the handle: the legal calls give a fresh handle's bits
        after = _legal_calls(used, mag_h, mag129_h, sig_h)
        clean = _legal_calls(fresh, mag_h, mag129_h, sig_h)
        assert len(after) == len(clean) == 12
        for i, (x, y) in enumerate(zip(after, clean)):
            assert np.isfinite(x).all() and np.abs(x).max() > 0, i
            assert x.tobytes() == y.tobytes(), i
    finally:
        used.close()
        fresh.close()
