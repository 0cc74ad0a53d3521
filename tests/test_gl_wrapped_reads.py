"""The three read paths of the streaming Griffin-Lim kernel's forward-transform input (griffin_lim.hip, fft_input), emulated
in numpy: the ring arithmetic of tests/test_host_logic.py::test_stream_ring_emulation restated with the kernel's three-way
decision -- linear, wrapped linear (an interior frame whose span crosses the end of the ring after the next lap's fold) and
index-mapped (reflect padding only) -- and the wrapped path's per-slot classification."""
import numpy as np
import pytest

NFFT, MH = 2048, 1024

CASES = [
    (1102, 275, 200, 1), (1102, 275, 75, 3), (1102, 275, 40, 2), (1024, 256, 40, 1), (1024, 256, 130, 3), (2048, 512, 100, 2),
    (400, 100, 150, 1), (64, 8, 300, 1), (2048, 1024, 30, 1), (1000, 250, 90, 2), (1101, 275, 50, 1), (2, 1, 700, 1),
    (1500, 1400, 20, 1), (2047, 256, 60, 1), (1200, 300, 70, 3), (800, 200, 130, 3), (800, 200, 45, 1),
    (1102, 275, 300, 3),
]
# utterances too short for their ring of R = 64 frames to come round (T + halo + lag indices <= R): no span is read after a fold
NO_WRAP = {(1024, 256, 40, 1), (800, 200, 45, 1), (1101, 275, 50, 1)}


def _ring_frames(win, hop, n_stage=1):
    """gl_stream_ring_frames (griffin_lim.hip) restated."""
    wpad = (NFFT - win) >> 1
    c_lo = wpad >> 7
    S = 128 * (((wpad + win - 1) >> 7) - c_lo + 1)
    acc = S - hop
    if acc < 0:
        return 0
    halo = -(-win // hop) - 1
    lag = halo if (halo + 1) * hop > 2 * (MH - wpad) else halo + 1
    budget = (160 * 1024 - 8 * 1088 * 8 - 64) // 4 // n_stage - acc - 132
    need = max(9 + lag + -(-S // hop) + 1, -(-(S + win + 2 * hop) // hop), 8)
    R = min(budget // hop, max(64, need))
    return R if R >= need else 0


def _read_span(ring, p0, n_sl, ring_len, folded, slots):
    """The kernel's linear read of a span that starts at ring position p0.  Lane l of slot j holds span samples
    128 j + 2 l + e.  One base per PAIR of slots (the odd slot is read 128 floats behind the even one); after the fold the
    pairs from slot j_sel on take their base ring_len lower, and slot j_sel itself -- the first one that is not wholly below
    the end of the ring -- is read again with an address per element.  `slots` counts the classes."""
    S = 128 * n_sl
    lane2 = 2 * np.arange(64)
    out = np.zeros(S)
    j_sel = (ring_len - p0) >> 7 if folded else 1 << 24
    for k in range((n_sl + 1) // 2):
        base = p0 + 256 * k - (ring_len if 2 * k >= j_sel else 0)
        for j in (2 * k, 2 * k + 1):
            if j >= n_sl:
                continue
            pos = base + 128 * (j & 1) + lane2
            if j != j_sel:   # (the kernel reads slot j_sel here as well and overwrites what it got)
                out[128 * j + lane2] = ring[pos]
                out[128 * j + lane2 + 1] = ring[pos + 1]
    if j_sel < n_sl:
        for e in range(2):
            pos = p0 + 128 * j_sel + lane2 + e
            out[128 * j_sel + lane2 + e] = ring[np.where(pos >= ring_len, pos - ring_len, pos)]
    # the classification that the base and the select amount to: a slot wholly below the end of the ring is read where it
    # is, one wholly at or above it ring_len lower, and the one that straddles it element by element
    ref = np.zeros(S)
    for j in range(n_sl):
        P = p0 + 128 * j
        if not folded or P + 128 <= ring_len:
            ref[128 * j:128 * j + 128] = ring[P:P + 128]
            slots['below'] += 1
        elif P >= ring_len:
            ref[128 * j:128 * j + 128] = ring[P - ring_len:P - ring_len + 128]
            slots['above'] += 1
        else:
            n = ring_len - P
            ref[128 * j:128 * j + n] = ring[P:ring_len]
            ref[128 * j + n:128 * j + 128] = ring[:128 - n]
            slots['straddle'] += 1
            assert j == j_sel
    assert np.array_equal(out, ref, equal_nan=True)
    return out


def _emulate(win, hop, T, n_stage):
    """-> path counts {'linear', 'wrapped', 'indexed', 'indexed_non_edge', 'old_indexed_non_edge', 'interior'} and the
    slot classes of the wrapped reads, over the whole utterance as one run and over the utterance cut into runs"""
    R = _ring_frames(win, hop, n_stage)
    assert R > 0
    ncol = -(-win // hop)
    halo = ncol - 1
    wpad = (NFFT - win) >> 1
    c_lo = wpad >> 7
    n_sl = ((wpad + win - 1) >> 7) - c_lo + 1
    S, fs = 128 * n_sl, 128 * c_lo
    acc, ring_len, w2 = S - hop, hop * R, MH - wpad
    lag = halo if (halo + 1) * hop > 2 * w2 else halo + 1
    Ltot = hop * (T - 1)
    rng = np.random.default_rng(win + hop)
    fr = np.zeros((T, NFFT))
    fr[:, wpad:wpad + win] = rng.standard_normal((T, win))
    full = np.zeros(hop * (T - 1) + NFFT)
    for t in range(T):
        full[t * hop:t * hop + NFFT] += fr[t]
    ytrim = full[MH:MH + Ltot]
    count = dict(linear=0, wrapped=0, indexed=0, indexed_non_edge=0, old_indexed_non_edge=0, interior=0)
    slots = dict(below=0, above=0, straddle=0)

    def frame_input(tm):
        y = tm * hop + np.arange(wpad, wpad + win) - MH
        y = np.where(y < 0, -y, y)
        y = np.where(y >= Ltot, 2 * (Ltot - 1) - y, y)
        out = np.zeros(NFFT)
        out[wpad:wpad + win] = ytrim[y]
        return out

    def run(t0, Lrun):
        ring = np.full(ring_len + acc + 128, np.nan)
        ring[ring_len:] = 0
        n_idx = Lrun + halo + lag
        y_base = (t0 - halo) * hop - MH + fs
        for i in range(n_idx):
            t, s = t0 - halo + i, i % R
            v = fr[t] if 0 <= t < T else np.zeros(NFFT)
            wr = hop * s
            rd = wr + (ring_len if s == 0 else 0)
            old = np.zeros(S)
            old[:acc] = ring[rd:rd + acc]
            ring[wr:wr + S] = old + v[fs:fs + S]
            if halo + lag <= i < halo + lag + Lrun:
                m, tm, sm = i - lag, t - lag, (s - lag) % R
                ylo = tm * hop + wpad - MH
                edge = ylo < 0 or ylo + win > Ltot
                crosses = hop * sm + S > ring_len
                folded = crosses and R - sm <= lag
                got = np.zeros(NFFT)
                if not edge:
                    count['interior'] += 1
                    count['old_indexed_non_edge'] += not (not crosses or R - sm > lag)
                    count['wrapped' if folded else 'linear'] += 1
                    got[fs:fs + S] = _read_span(ring, hop * sm, n_sl, ring_len, folded, slots if folded else dict(slots))   # (classes of wrapped reads only)
                    got[:wpad] = 0
                    got[wpad + win:] = 0
                else:
                    count['indexed'] += 1
                    count['indexed_non_edge'] += not edge
                    lap0 = m // R
                    for f in range(wpad, wpad + win):
                        y = ylo + (f - wpad)
                        y = -y if y < 0 else y
                        y = 2 * (Ltot - 1) - y if y >= Ltot else y
                        off, lap = (y - y_base) - lap0 * ring_len, lap0
                        if off >= ring_len:
                            off, lap = off - ring_len, lap + 1
                        elif off < 0:
                            off, lap = off + ring_len, lap - 1
                        assert 0 <= off < ring_len
                        got[f] = ring[ring_len + off if (off < acc and lap * R > i) else off]
                assert np.allclose(got, frame_input(tm), atol=1e-12), (tm, i, edge, folded)

    run(0, T)
    L1 = max(8, T // 3 // 8 * 8)
    for t0 in range(0, T, L1):
        run(t0, min(L1, T - t0))
    return count, slots


@pytest.fixture(scope='module')
def emulated():
    return {c: _emulate(*c) for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(map(str, c)))
def test_every_transform_input_is_the_overlap_added_signal(emulated, case):
    """(asserted frame by frame inside the emulation) -- and every frame took exactly one of the three paths, the
    index-mapped one only where the window leaves the signal"""
    count, _ = emulated[case]
    assert count['indexed_non_edge'] == 0
    assert count['linear'] + count['wrapped'] == count['interior'] > 0
    assert count['indexed'] > 0


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(map(str, c)))
def test_wrapped_path_takes_what_the_index_mapped_path_took_of_the_interior(emulated, case):
    count, slots = emulated[case]
    assert count['wrapped'] == count['old_indexed_non_edge']
    if case in NO_WRAP:
        assert count['wrapped'] == 0
    else:
        assert count['wrapped'] >= 1
        # every wrapped span reaches the end of the ring, and at most one of its slots straddles it
        assert slots['straddle'] <= count['wrapped'] <= slots['above'] + slots['straddle']
        assert sum(slots.values()) % count['wrapped'] == 0   # (n_sl slots each)
    if case == (1102, 275, 300, 3):
        assert (count['wrapped'], count['interior']) == (96, 588)
