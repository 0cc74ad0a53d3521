"""GPU parity: HIP network stages (through the C ABI) vs the float64 numpy oracle.

Tolerance: BASELINE.json's north star asks for spectrograms within 1e-3 rel-L2 of the CPU
reference; stage intermediates are held to 1e-4 (fp32 MFMA vs fp64), final outputs to 1e-3.
"""
import os

import numpy as np
import pytest

from conftest import pkg, rel_l2
from parity import BTC, assert_alignment_rows, assert_mel_parity, assert_parity
from oracle import tacotron_oracle as O

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
FINAL_TOL = 1e-3


def make_ids(rng, B, Ts):
    ids = rng.integers(2, 39, (B, Ts)).astype(np.int32)
    for b in range(B):
        L = int(rng.integers(max(2, Ts // 2), Ts))
        ids[b, L - 1] = 1
        ids[b, L:] = 0
    return ids


# Ts % 3 = 1, 2, 1, 0: the bi-GRU loop is unrolled by three (gru.hip), every remainder is walked
@pytest.mark.parametrize('B,Ts', [(2, 7), (4, 8), (3, 37), (5, 150)])
def test_encoder_stages(engine, hparams, weights64, B, Ts):
    rng = np.random.default_rng(100 + B)
    ids = make_ids(rng, B, Ts)
    stages = {}
    ref = O.encoder(ids, weights64, hparams, stages)
    mem = engine.encoder_forward(ids).to_host()
    M = B * Ts
    got = {
        'prenet': engine.debug_workspace('enc.pre2', (B, Ts, 128)),
        'bank': engine.debug_workspace('enc.bank', (B, Ts, 2048)),
        'proj1': engine.debug_workspace('enc.p1', (B, Ts, 128)),
        'proj2': engine.debug_workspace('enc.p2', (B, Ts, 128)),
        'highway': engine.debug_workspace('enc.hw0', (B, Ts, 128)),
    }
    refs = {k: stages[k] if k != 'proj2' else stages['proj2'] + stages['prenet'] for k in got}
    errs = {k: rel_l2(v, refs[k]) for k, v in got.items()}
    errs['memory'] = rel_l2(mem, ref)
    print('encoder B={} Ts={}: {}'.format(B, Ts, errs))
    for k, e in errs.items():
        assert e < (FINAL_TOL if k == 'memory' else STAGE_TOL), (k, e)
    label = 'encoder B={} Ts={}'.format(B, Ts)
    for k, v in got.items():
        assert_parity(v, refs[k], BTC, STAGE_TOL, '{} {}'.format(label, k))
    assert_parity(mem, ref, BTC, FINAL_TOL, label + ' memory')


@pytest.mark.parametrize('B,Ts,S', [(2, 7, 3), (3, 37, 10), (17, 150, 6)])
def test_decoder(engine, hparams, weights64, B, Ts, S):
    rng = np.random.default_rng(200 + B)
    # sharper attention than random-init memory gives: scale up
    memory = (rng.standard_normal((B, Ts, 256)) * 1.5).astype(np.float32)
    ref_mel, ref_al = O.decoder(memory.astype(np.float64), weights64, hparams, n_steps=S)
    mel, al = engine.decoder_forward(memory, S)
    e_mel, e_al = rel_l2(mel.to_host(), ref_mel), float(np.abs(al.to_host() - ref_al).max())
    print('decoder B={} Ts={} S={}: mel rel-L2 {:.3e}, align max-abs {:.3e}, align peak {:.3f}'.format(
        B, Ts, S, e_mel, e_al, float(ref_al.max())))
    assert e_mel < FINAL_TOL
    assert e_al < 1e-4
    assert np.allclose(al.to_host().sum(-1), 1.0, atol=1e-5)
    label = 'decoder B={} Ts={} S={}'.format(B, Ts, S)
    assert_mel_parity(mel.to_host(), ref_mel, FINAL_TOL, label)
    assert_alignment_rows(al.to_host(), ref_al, 1e-4, label)


def test_decoder_graph_matches_eager(engine):
    """Option "use_graph": the launch-per-layer decoder loop replayed from a cached hipGraph gives the bits of the directly
    enqueued launches -- on the HIP runtime the library was built with.  A process that loaded an older libamdhip64 first (this
    suite's collection imports torch, which bundles HIP 7.0) is refused the option: replays were wrong there (csrc/api_internal.h, `use_graph`)."""
    rng = np.random.default_rng(7)
    memory = engine.to_device((rng.standard_normal((4, 21, 256))).astype(np.float32))
    engine.set_option('use_graph', 0)
    mel0, al0 = engine.decoder_forward(memory, 5)
    m0, a0 = mel0.to_host(), al0.to_host()
    try:
        try:
            engine.set_option('use_graph', 1)
        except pkg('_hip').TtsError as e:
            assert e.code == pkg('_hip').TTS_ERR_UNSUPPORTED and 'HIP runtime' in str(e)
            return
        mel1, al1 = engine.decoder_forward(memory, 5)
        # replay the cached graph into the same buffers
        engine.decoder_forward(memory, 5, mel=mel1, alignments=al1)
        assert np.array_equal(m0, mel1.to_host())
        assert np.array_equal(a0, al1.to_host())
    finally:
        engine.set_option('use_graph', 0)


def test_decoder_graph_in_a_process_of_its_own():
    """The sequence that showed the graph problem (a cached decoder graph replayed between calls of the persistent decoder,
    serial and pipelined, after calls of another shape: tools/graph_probe.py), in a fresh interpreter that has NOT imported
    torch -- i.e. on /opt/rocm's runtime, where the option is allowed: every graph call equals the directly enqueued one."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for prelude in (2, 3):
        r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'graph_probe.py'), '--reps', '3', '--prelude', str(prelude)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert 'serial with use_graph=1: 0 of 3' in r.stdout and 'pipelined with use_graph=1: 0 of 3' in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize('B,T', [(2, 15), (2, 20), (3, 100)])   # T % 3 = 0, 2, 1
def test_postnet_stages(engine, hparams, weights64, B, T):
    rng = np.random.default_rng(300 + B)
    mel = rng.random((B, T, 80)).astype(np.float32)
    stages = {}
    ref = O.post_process(mel.astype(np.float64), weights64, hparams, stages)
    lin = engine.postnet_forward(mel).to_host()
    got = {
        'bank': engine.debug_workspace('post.bank', (B, T, 1024)),
        'proj1': engine.debug_workspace('post.p1', (B, T, 256)),
        'highway': engine.debug_workspace('post.hw0', (B, T, 128)),
        'gru': engine.debug_workspace('post.gru', (B, T, 256)),
    }
    errs = {k: rel_l2(v, stages[k]) for k, v in got.items()}
    errs['linear'] = rel_l2(lin, ref)
    print('postnet B={} T={}: {}'.format(B, T, errs))
    for k, e in errs.items():
        assert e < (FINAL_TOL if k in ('linear', 'gru') else STAGE_TOL), (k, e)
    label = 'postnet B={} T={}'.format(B, T)
    for k, v in got.items():
        assert_parity(v, stages[k], BTC, FINAL_TOL if k == 'gru' else STAGE_TOL, '{} {}'.format(label, k))
    assert_parity(lin, ref, BTC, FINAL_TOL, label + ' linear')


def test_full_network_small(engine, hparams, weights64):
    rng = np.random.default_rng(5)
    ids = make_ids(rng, 2, 11)
    ref = O.tacotron_predict(ids, weights64, hparams, n_steps=4)
    mem = engine.encoder_forward(ids)
    mel, al = engine.decoder_forward(mem, 4)
    B = 2
    lin = engine.postnet_forward(mel.to_host().reshape(B, -1, 80))
    assert rel_l2(mel.to_host(), ref['reduced_mel']) < FINAL_TOL
    assert rel_l2(lin.to_host(), ref['linear']) < FINAL_TOL
    assert_parity(mem.to_host(), ref['memory'], BTC, FINAL_TOL, 'full network memory')
    assert_mel_parity(mel.to_host(), ref['reduced_mel'], FINAL_TOL, 'full network')
    assert_alignment_rows(al.to_host(), ref['alignments'], 1e-4, 'full network')
    assert_parity(lin.to_host(), ref['linear'], BTC, FINAL_TOL, 'full network linear')


# ---- CBHG tail (csrc/cbhg_tail.hip): lifter + highway stack + GRU input projections in one launch, against the oracle and
# against the layer-by-layer GEMM chain it replaces
@pytest.mark.parametrize('fused', [1, 0])
@pytest.mark.parametrize('B,T', [(1, 1), (2, 63), (3, 129), (5, 200)])   # one row, a partial tile, tile + 1 row + remainder, several tiles
def test_cbhg_tail_forms(engine, hparams, weights64, fused, B, T):
    rng = np.random.default_rng(900 + B)
    mel = rng.random((B, T, 80)).astype(np.float32)
    stages = {}
    ref = O.post_process(mel.astype(np.float64), weights64, hparams, stages)
    engine.set_option('fused_tail', fused)
    try:
        lin = engine.postnet_forward(mel).to_host()
        hw = engine.debug_workspace('post.hw0', (B, T, 128))
        gru = engine.debug_workspace('post.gru', (B, T, 256))
    finally:
        engine.set_option('fused_tail', 1)
    e = {'highway': rel_l2(hw, stages['highway']), 'gru': rel_l2(gru, stages['gru']), 'linear': rel_l2(lin, ref)}
    print('cbhg tail fused={} B={} T={}: {}'.format(fused, B, T, e))
    assert e['highway'] < STAGE_TOL and e['gru'] < FINAL_TOL and e['linear'] < FINAL_TOL, e
    label = 'cbhg tail fused={} B={} T={}'.format(fused, B, T)
    assert_parity(hw, stages['highway'], BTC, STAGE_TOL, label + ' highway')
    assert_parity(gru, stages['gru'], BTC, FINAL_TOL, label + ' gru')
    assert_parity(lin, ref, BTC, FINAL_TOL, label + ' linear')


@pytest.mark.parametrize('n_hw', [0, 1, 3])
def test_cbhg_tail_layer_counts(hparams, n_hw):
    """other highway depths than the reference's four (layers.py:546-558 takes any): encoder (128-wide input, the lifter sees
    full k-chunks) and post-net (80-wide: a padded chunk) against the oracle"""
    import copy
    hp = copy.deepcopy(hparams)
    hp.encoder.n_highway_layers = n_hw
    hp.post.n_highway_layers = n_hw
    w = pkg('tacotron.weights').synthetic_weights(3, hp)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    eng = pkg().Engine(hp)
    try:
        eng.load_weights(w)
        rng = np.random.default_rng(n_hw)
        ids = make_ids(rng, 3, 50)
        mem = eng.encoder_forward(ids).to_host()
        ref_mem = O.encoder(ids, w64, hp, {})
        assert rel_l2(mem, ref_mem) < FINAL_TOL
        mel = rng.random((2, 70, 80)).astype(np.float32)
        st = {}
        ref = O.post_process(mel.astype(np.float64), w64, hp, st)
        lin = eng.postnet_forward(mel).to_host()
        hw = eng.debug_workspace('post.hw0', (2, 70, 128))
        assert rel_l2(hw, st['highway']) < STAGE_TOL
        assert rel_l2(lin, ref) < FINAL_TOL
        label = 'cbhg tail n_hw={}'.format(n_hw)
        assert_parity(mem, ref_mem, BTC, FINAL_TOL, label + ' memory')
        assert_parity(hw, st['highway'], BTC, STAGE_TOL, label + ' highway')
        assert_parity(lin, ref, BTC, FINAL_TOL, label + ' linear')
    finally:
        eng.close()
