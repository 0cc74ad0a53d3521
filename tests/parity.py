"""Per-slice parity checks for the network and GEMM tests (a plain helper module, imported like conftest's helpers).

One rel-L2 over a whole batch tensor dilutes an error that sits in one slice -- one utterance, one output column of a GEMM,
one frame -- by the square root of the number of slices, and the kernels cut their work into exactly such slices (clusters
of utterances, N tiles, time tiles, the decoder's last steps).  These helpers hold every slice along each named axis to
the test's bound:

    err_i = |g_i - r_i| / max(|r_i|, |r| / sqrt(n_axis))

The floor is the RMS slice norm: a slice whose reference is (nearly) zero -- padded frames, dead channels -- is measured
against a typical slice instead of dividing by ~0, and still fails if its error is large compared with that.  An
elementwise figure, max|g - r| / max|r|, is held to the same bound.
"""
import numpy as np


def slice_errors(got, ref, axes):
    """{name: (worst slice error, index of that slice)} for every name -> axis of `axes`, plus
    'elem': (max|g - r| / max|r|, index of the worst element)."""
    g = np.asarray(got, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    d = g - r
    total = np.linalg.norm(r)
    out = {}
    for name, ax in axes.items():
        ax = ax % r.ndim
        others = tuple(i for i in range(r.ndim) if i != ax)
        n = r.shape[ax]
        num = np.sqrt(np.sum(d * d, axis=others))
        den = np.maximum(np.sqrt(np.sum(r * r, axis=others)), total / np.sqrt(n))
        e = num / np.maximum(den, 1e-300)
        i = int(np.argmax(e))
        out[name] = (float(e[i]), i)
    ad = np.abs(d)
    i = np.unravel_index(int(np.argmax(ad)), ad.shape)
    out['elem'] = (float(ad[i] / max(float(np.abs(r).max()), 1e-300)), tuple(int(k) for k in i))
    return out


def assert_parity(got, ref, axes, tol, label):
    """Print the worst slice per axis (and the elementwise figure) on one line each, then hold all of them to `tol`."""
    errs = slice_errors(got, ref, axes)
    for name, (e, i) in errs.items():
        print('parity {} {}: worst {:.3e} at {} (bound {:.0e})'.format(label, name, e, i, tol))
    bad = {name: v for name, v in errs.items() if not v[0] < tol}
    assert not bad, (label, tol, bad)
    return errs


def assert_segment_parity(got, ref, hop, tol, label):
    """A waveform [hop (T - 1)] (or a batch [B, hop (T - 1)] of them) as its hop segments [T - 1, hop]: every segment --
    the two at the ends of an utterance, where the halo and the window sum differ, and the ones at the seams between runs
    among them -- and every sample to `tol`, with the floor of slice_errors (a silent segment is measured against the
    RMS one)."""
    g = np.asarray(got)
    r = np.asarray(ref)
    assert g.shape == r.shape and r.shape[-1] % hop == 0, (g.shape, r.shape, hop)
    if r.ndim == 1:
        return assert_parity(g.reshape(-1, hop), r.reshape(-1, hop), {'seg': 0}, tol, label)
    B = r.shape[0]
    return assert_parity(g.reshape(B, -1, hop), r.reshape(B, -1, hop), {'utt': 0, 'seg': 1}, tol, label)


def alignment_rows(got, ref):
    """rel-L2 of every (step, utterance) row of [S, B, Ts] alignments, as an [S, B] array.  A row of softmax weights sums
    to 1, so its norm is at least 1 / sqrt(Ts): no floor is needed (an all-zero reference row -- nothing to attend to --
    is measured in absolute terms)."""
    g = np.asarray(got, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    assert g.shape == r.shape and r.ndim == 3, (g.shape, r.shape)
    return np.linalg.norm(g - r, axis=-1) / np.maximum(np.linalg.norm(r, axis=-1), 1e-300)


def assert_alignment_rows(got, ref, tol, label):
    """Print the worst alignment row and hold every row's rel-L2 to `tol`."""
    e = alignment_rows(got, ref)
    s, b = np.unravel_index(int(np.argmax(e)), e.shape)
    worst = float(e[s, b])
    print('parity {} align rows: worst {:.3e} at step {} utt {} (bound {:.0e})'.format(label, worst, s, b, tol))
    assert worst < tol, (label, tol, worst, (int(s), int(b)))
    return worst


def assert_mel_parity(got, ref, tol, label, n_mels=80):
    """Reduced mel [B, S, r * n_mels]: per utterance, decoder step and GEMM column, and again as [B, r S, n_mels]
    frames x mel channels."""
    g = np.asarray(got)
    r = np.asarray(ref)
    assert_parity(g, r, {'utt': 0, 'step': 1, 'col': 2}, tol, label + ' mel')
    B = r.shape[0]
    assert_parity(g.reshape(B, -1, n_mels), r.reshape(B, -1, n_mels), {'utt': 0, 'frame': 1, 'chan': 2}, tol,
                  label + ' mel frames')


# the [B, T, C] layout of the memory, stage workspaces, mel frames and linear spectrograms
BTC = {'utt': 0, 'frame': 1, 'chan': 2}
