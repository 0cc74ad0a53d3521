"""What the tests of the segment-wise stages share (a plain helper module; warp_cases, shift_cases and resample_segments_cases
re-export it under their own names): the pattern `out` holds before a call, a list's rows as the record array the library reads,
and a batch whose frames behind its lengths must never be read."""
import numpy as np

NAN_PATTERN = 0x7fc0beef            # what `out` holds before every call: a NaN no computation makes


def segment_array(dtype, segments):
    """the rows as the contiguous array of the record ``dtype`` the library reads (unchecked: refusals travel through it too); a row
    either has every field, or leaves out ``reserved``, which is then 0"""
    q = np.zeros(len(segments), dtype=dtype)
    at = dtype.names.index('reserved') if 'reserved' in dtype.names else None
    for s, r in enumerate(segments):
        q[s] = tuple(r) if len(r) == len(dtype.names) else tuple(r[:at]) + (0,) + tuple(r[at:])
    return q


def poisoned(x, n_frames):
    """x (B, F, T) with a NaN in every frame at or behind n_frames[b]: what the kernel must never read (it would show as NaN)"""
    y = x.copy()
    if n_frames is not None:
        for b, n in enumerate(n_frames):
            y[b, :, n:] = np.nan
    return y
