"""GPU: the real `bench.py --gpus 2` path, launched without torchrun.  With one GPU in the box the two ranks
share it (SSTTS_DIST_BACKEND=gloo: RCCL needs one device per rank); what is checked is the launcher, the weight
broadcast, the per-rank shards and the max-over-ranks timing -- not a scaling number."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_gpus2_self_launch_gloo():
    env = dict(os.environ, SSTTS_DIST_BACKEND='gloo')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
                          '--full', '--no-cpu-baseline'], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    rec = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith('{')][-1])
    assert rec['n_gpus'] == 2 and rec['world_size_seen'] == 2
    assert rec['config']['global_batch'] == 128 and rec['scaling'] == 'weak'
    assert rec['value'] > 0 and rec['steps'] == 2
    # the N > 1 diagnostics: every rank's own time with the straggler named, both broadcasts, one device record per rank
    # (the two gloo ranks share the one device of the box: same uuid twice, allowed under gloo only), the padded length
    assert len(rec['rank_ms_per_step']) == 2 and all(t > 0 for t in rec['rank_ms_per_step'])
    assert rec['straggler_rank'] in (0, 1) and rec['rank_ms_per_step_max'] == max(rec['rank_ms_per_step'])
    assert rec['rank_ms_per_step_max'] <= rec['ms_per_step'] * 1.05
    assert rec['weight_broadcast_ms'] > 0 and rec['weight_broadcast_ms_steady'] > 0 and rec['communicator_setup_ms'] > 0
    assert len(rec['rank_devices']) == 2 and all(len(d['uuid']) == 32 and d['compute_units'] > 0 for d in rec['rank_devices'])
    assert rec['padded_sentence_length'] == 150
    for key in ('roofline', 'roofline_valu', 'roofline_decoder', 'roofline_mfma'):
        assert key in rec
    # --full: the measurements that take runs of their own after the timed steps, on every rank of the N > 1 path
    assert rec['full'] is True and rec['roofline_mfma']['achieved'] > 0 and rec['roofline']['iteration_ms_alone'] > 0


def test_bench_under_torchrun_one_rccl_rank():
    """The driver's launch line (python -m torch.distributed.run ... bench.py --gpus N) with the `nccl` = RCCL backend, as
    far as a one-GPU box allows: ONE rank (two RCCL ranks cannot share a device), SSTTS_DIST_SINGLE=1 makes bench.py bring
    the process group up anyway -- communicator set-up, the weight broadcast from a device tensor, barriers around the timed
    region and the max all-reduce all run on RCCL beside the library's own streams."""
    env = dict(os.environ, SSTTS_DIST_SINGLE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('SSTTS_DIST_BACKEND', None)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1',
                          '--master-addr', '127.0.0.1', '--master-port', '29533', os.path.join(ROOT, 'bench.py'),
                          '--gpus', '1', '--steps', '3', '--warmup', '1', '--no-cpu-baseline'],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    err = out.stderr.decode()
    if out.returncode != 0 and 'process group up' not in err and ('NCCL' in err or 'RCCL' in err or 'ncclSystemError' in err):
        pytest.skip('RCCL could not bring up a communicator on this box: ' + err[-400:])   # the box's fault, not the path's
    assert out.returncode == 0, err[-3000:]
    assert 'backend nccl world size 1' in err
    rec = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith('{')][-1])
    assert rec['n_gpus'] == 1 and rec['world_size_seen'] == 1 and rec['weight_broadcast_ms'] is not None
    assert rec['weight_broadcast_ms_steady'] > 0 and rec['communicator_setup_ms'] > 0
    assert rec['rank_ms_per_step'] and len(rec['rank_devices']) == 1 and rec['straggler_rank'] == 0
    assert rec['value'] > 0 and rec['steps'] == 3
    # a plain run: none of the measurements --full adds
    assert rec['full'] is False and rec['roofline_mfma'] is None and rec['cpu_baseline'] is None


def test_bench_dump_outputs(tmp_path):
    """`bench.py --dump-outputs DIR`: what the last timed step returned, float32, at most 64 MB, the same from run to run
    with the same arguments (same inputs, same seeds) -- what lets two builds be compared output for output."""
    import numpy as np
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = tmp_path / 'run{}'.format(run)
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--no-cpu-baseline',
                              '--dump-outputs', str(d)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert out.returncode == 0, out.stderr.decode()[-3000:]
        rec = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith('{')][-1])
        assert rec['steps'] == 2
        dumps.append({p.stem: np.load(str(p)) for p in d.glob('*.npy')})
    a = dumps[0]
    assert set(a) == {'utterances', 'wav', 'linear', 'alignments'}
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    n = a['utterances'].shape[0]
    assert a['wav'].shape == (n, 275 * 999) and a['linear'].shape == (n, 1000, 1025) and a['alignments'].shape == (200, 64, 150)
    assert a['alignments'].min() >= 0.0 and a['alignments'].max() <= 1.0 + 1e-6   # attention weights of every decoder step
    assert 0.99 < float(np.abs(a['wav']).max()) <= 1.0 + 1e-6            # peak-normalised waveforms
    for k in a:
        assert np.array_equal(a[k], dumps[1][k]), k
